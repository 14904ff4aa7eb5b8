// gs_rigid_fit and gs_model_transform_compose under AddressSanitizer + UBSan on the CPU: the host arithmetic
// of csrc/gs_align_fit.h, the header gs_align.hip wraps into the C ABI, compiled alone into this stand-alone program.  Every
// record lives in a heap block of exactly its size, so a read or write beside it is caught; the inputs are well-posed fits,
// every refusal of the header, and hostile sums (NaN, infinities, huge and tiny magnitudes, zeros).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../../wgpu-3dgs-core_amd/csrc/gs_align_fit.h"

#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static uint32_t lcg(uint32_t &s) { return s = s * 1664525u + 1013904223u; }
static double unit(uint32_t &s) { return (double)(lcg(s) >> 8) * (1.0 / 16777216.0) * 2.0 - 1.0; }

// the sums of n pairs q = s R p + t (+ noise), R from the quaternion (w, x, y, z)
static void sums_of(uint32_t &seed, int n, const double quat[4], double scale, const double t[3], double noise, gs_pair_sums *out) {
    double R[3][3];
    gsfit::quat_matrix(quat, R);
    std::memset(out, 0, sizeof(*out));
    for (int i = 0; i < n; i++) {
        double p[3], q[3];
        for (int a = 0; a < 3; a++) p[a] = (double)(float)(2.0 * unit(seed));
        for (int a = 0; a < 3; a++) q[a] = (double)(float)(scale * (R[a][0] * p[0] + R[a][1] * p[1] + R[a][2] * p[2]) + t[a] + noise * unit(seed));
        out->pairs++;
        for (int a = 0; a < 3; a++) {
            out->sp[a] += p[a];
            out->sq[a] += q[a];
            for (int b = 0; b < 3; b++) out->spq[3 * a + b] += p[a] * q[b];
            out->spp += p[a] * p[a];
            out->sqq += q[a] * q[a];
            out->sdd += (p[a] - q[a]) * (p[a] - q[a]);
        }
    }
}

int main() {
    uint32_t seed = 99u;
    int fits = 0, refusals = 0;
    for (int round = 0; round < 400; round++) {
        std::unique_ptr<gs_pair_sums> sums(new gs_pair_sums);
        std::unique_ptr<gs_model_transform_pod> delta(new gs_model_transform_pod), m(new gs_model_transform_pod), out(new gs_model_transform_pod);
        std::unique_ptr<double> rms(new double(-1.0));
        double quat[4] = {unit(seed), unit(seed), unit(seed), unit(seed)};
        const double len = std::sqrt(quat[0] * quat[0] + quat[1] * quat[1] + quat[2] * quat[2] + quat[3] * quat[3]);
        if (len < 0.1) continue;
        for (double &v : quat) v /= len;
        if (quat[0] < 0.0) for (double &v : quat) v = -v;
        const double scale = round % 2 ? 0.5 + std::fabs(unit(seed)) : 1.0, t[3] = {3.0 * unit(seed), 3.0 * unit(seed), 3.0 * unit(seed)};
        sums_of(seed, 3 + round % 60, quat, scale, t, round % 3 ? 0.0 : 0.01, sums.get());
        std::memset(delta.get(), 0xee, sizeof(*delta));
        const char *why = gsfit::rigid_fit(sums.get(), round % 2, delta.get(), round % 5 ? rms.get() : nullptr);
        if (why) { refusals++; continue; }      // (three or four pairs may be degenerate)
        fits++;
        if (round % 3 && sums->pairs >= 8) {      // noise-free: the transform comes back to binary32
            REQUIRE(std::fabs(delta->rot[3] - quat[0]) < 1e-4 && std::fabs(delta->rot[0] - quat[1]) < 1e-4);
            REQUIRE(std::fabs(delta->scale[0] - scale) < 1e-4 && std::fabs(delta->pos[0] - t[0]) < 1e-3);
        }
        REQUIRE(delta->rot[3] >= 0.0f && delta->_pad0 == 0.0f && delta->_pad1 == 0.0f);
        const float pos[3] = {(float)unit(seed), (float)unit(seed), (float)unit(seed)}, rot[4] = {0.5f, -0.5f, 0.5f, 0.5f}, sc[3] = {1.25f, 0.75f, 2.0f};
        std::memcpy(m->pos, pos, 12); std::memcpy(m->rot, rot, 16); std::memcpy(m->scale, sc, 12);
        m->_pad0 = m->_pad1 = 0.0f;
        gsfit::compose(delta.get(), m.get(), out.get());
        REQUIRE(std::fabs(out->scale[1] - delta->scale[0] * 0.75f) < 1e-6);
        gsfit::compose(delta.get(), m.get(), m.get());      // in place
        REQUIRE(std::memcmp(out.get(), m.get(), sizeof(*out)) == 0);
    }
    REQUIRE(fits > 300);
    // every refusal, and hostile sums: nothing is written, nothing traps
    const double hostile[] = {0.0, -0.0, NAN, INFINITY, -INFINITY, 1e308, -1e308, 1e-320, 4.9e-324, 1.0, -1.0, 1e154, 1e-154};
    const int nh = (int)(sizeof(hostile) / sizeof(hostile[0]));
    for (int round = 0; round < 20000; round++) {
        std::unique_ptr<gs_pair_sums> sums(new gs_pair_sums);
        std::unique_ptr<gs_model_transform_pod> delta(new gs_model_transform_pod);
        sums->pairs = round % 7 == 0 ? (uint64_t)(lcg(seed) % 4u) : round % 11 == 0 ? ~0ull : 1u + lcg(seed) % 1000u;
        double *d = sums->sp;
        for (int f = 0; f < 3; f++) sums->sp[f] = lcg(seed) % 3u ? unit(seed) * 100.0 : hostile[lcg(seed) % nh];
        for (int f = 0; f < 3; f++) sums->sq[f] = lcg(seed) % 3u ? unit(seed) * 100.0 : hostile[lcg(seed) % nh];
        for (int f = 0; f < 9; f++) sums->spq[f] = lcg(seed) % 3u ? unit(seed) * 100.0 : hostile[lcg(seed) % nh];
        sums->spp = lcg(seed) % 3u ? std::fabs(unit(seed)) * 1000.0 : hostile[lcg(seed) % nh];
        sums->sqq = lcg(seed) % 3u ? std::fabs(unit(seed)) * 1000.0 : hostile[lcg(seed) % nh];
        sums->sdd = lcg(seed) % 3u ? std::fabs(unit(seed)) * 1000.0 : hostile[lcg(seed) % nh];
        (void)d;
        std::memset(delta.get(), 0xee, sizeof(*delta));
        gs_model_transform_pod before;
        std::memcpy(&before, delta.get(), sizeof(before));
        const char *why = gsfit::rigid_fit(sums.get(), round & 1, delta.get(), nullptr);
        if (why) {
            refusals++;
            REQUIRE(std::memcmp(&before, delta.get(), sizeof(before)) == 0);
        } else {
            for (int a = 0; a < 4; a++) REQUIRE(std::isfinite(delta->rot[a]));
            gsfit::compose(delta.get(), delta.get(), delta.get());
        }
    }
    REQUIRE(refusals > 1000);
    std::printf("sanitize align fit OK (%d fits, %d refusals)\n", fits, refusals);
    return 0;
}
