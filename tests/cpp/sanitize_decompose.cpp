// CPU-only sanitizer harness of the covariance decomposition (tests/test_decompose_sanitizers.py): the host
// side of the functions gs_cov3d_decompose and gs_decompose_pods consist of, gs::cov3d_decompose and gs::decompose_words
// (csrc/gs_convert.h, csrc/gs_pack_kernels.h: the code the device kernel runs too), compiled with
//   hipcc --cuda-host-only -Xarch_host -fsanitize=address,undefined
// and run over the set of the decomposition tests — covariances packed from random rotations with scales log-uniform in
// [1e-4, 1e2] (two equal scales, isotropic, flat, nearly equal), raw indefinite matrices — and over hostile words.  Records
// live in heap blocks of exactly the record's size, so a word read or written past a record is an error.  Besides the
// sanitizers' own findings: every result of a finite input is finite, the quaternion has unit length and w >= 0.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../wgpu-3dgs-core_amd/csrc/gs_pack_kernels.h"

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static float host_sqrt(float v) { return std::sqrt(v); }

static int check_one(const float c[6]) {
    float q[4], s[3];
    gs::cov3d_decompose(c, q, s, host_sqrt);
    bool finite = true;
    for (int k = 0; k < 6; k++) finite = finite && std::isfinite(c[k]);
    for (int k = 0; k < 4; k++) REQUIRE(std::isfinite(q[k]));
    const double len2 = (double)q[0] * q[0] + (double)q[1] * q[1] + (double)q[2] * q[2] + (double)q[3] * q[3];
    REQUIRE(std::fabs(len2 - 1.0) <= 4.0 / 8388608.0 && q[3] >= 0.0f);
    for (int k = 0; k < 3; k++) REQUIRE(finite ? std::isfinite(s[k]) && s[k] >= 0.0f : gs::cv_f2u(s[k]) == 0x7fc00000u);
    return 0;
}

int main() {
    std::mt19937 rng(7);
    std::uniform_real_distribution<float> uni(-1.0f, 1.0f), unit(0.0f, 1.0f);
    std::normal_distribution<float> normal;
    std::vector<float> covs;
    for (int i = 0; i < 20000; i++) {
        float q[4], s[3], c[6];
        float len = 0.0f;
        for (int k = 0; k < 4; k++) { q[k] = normal(rng); len += q[k] * q[k]; }
        for (int k = 0; k < 4; k++) q[k] /= std::sqrt(len);
        for (int k = 0; k < 3; k++) s[k] = std::exp(std::log(1e-4f) + unit(rng) * (std::log(1e2f) - std::log(1e-4f)));
        const float kind = unit(rng);
        if (kind < 0.10f) s[1] = s[0];
        else if (kind < 0.20f) s[1] = s[2] = s[0];
        else if (kind < 0.25f) s[2] = 0.0f;
        else if (kind < 0.33f) s[1] = s[0] * (1.0f + 1e-6f);
        gs::cov3d_from_rot_scale(q, s, c);
        covs.insert(covs.end(), c, c + 6);
    }
    for (int i = 0; i < 2000 * 6; i++) covs.push_back(uni(rng));
    const float hostile[] = {0.0f, -0.0f, 1e-45f, 1e-38f, 1e-20f, 1.0f, 1e30f, 3.4028235e38f, -1.0f, INFINITY, -INFINITY, NAN};
    for (float a : hostile)
        for (float b : hostile) {
            const float c[6] = {a, b, 0.0f, a, b, b};
            covs.insert(covs.end(), c, c + 6);
            const float d[6] = {a, 0.0f, 0.0f, b, 0.0f, a};
            covs.insert(covs.end(), d, d + 6);
        }
    const size_t n = covs.size() / 6;
    for (size_t i = 0; i < n; i++)
        if (check_one(&covs[6 * i])) return 1;

    // records of the eight covariance layouts -> the four destination SH configs, and the rot-scale sources through the same entry
    for (int ssh = 0; ssh < 4; ssh++)
        for (int scov = 0; scov < 3; scov++)
            for (int dsh = 0; dsh < 4; dsh++) {
                if (scov == gs::COV_ROT_SCALE && ssh == dsh) continue;      // identical layouts are a copy, not this function
                const int sw = gs::pod_words(ssh, scov), dw = gs::pod_words(dsh, gs::COV_ROT_SCALE);
                for (size_t i = 0; i < n; i += 7) {
                    uint32_t g[gs::GAUSSIAN_WORDS];
                    for (int k = 0; k < gs::GAUSSIAN_WORDS; k++) g[k] = gs::cv_f2u(uni(rng));
                    uint32_t *p = (uint32_t *)std::malloc((size_t)sw * 4), *o = (uint32_t *)std::malloc((size_t)dw * 4);
                    gs::pack_words(ssh, scov, g, p);
                    uint32_t *c = p + gs::cov_word0(ssh);
                    if (scov == gs::COV_SINGLE)
                        std::memcpy(c, &covs[6 * i], 24);
                    else if (scov == gs::COV_HALF)
                        for (int k = 0; k < 3; k++)
                            c[k] = gs::f32_to_f16_rtne_bits(gs::cv_f2u(covs[6 * i + 2 * k])) |
                                   ((uint32_t)gs::f32_to_f16_rtne_bits(gs::cv_f2u(covs[6 * i + 2 * k + 1])) << 16);
                    std::memset(o, 0xAB, (size_t)dw * 4);
                    gs::decompose_words(ssh, scov, dsh, p, o, host_sqrt);
                    for (int k = gs::cov_word0(dsh) + 7; k < dw; k++) REQUIRE(o[k] == 0u);      // the trailing pad
                    REQUIRE(o[0] == p[0] && o[3] == p[3]);
                    std::free(p);
                    std::free(o);
                }
            }
    std::printf("sanitize decompose OK: %zu covariances\n", n);
    return 0;
}
