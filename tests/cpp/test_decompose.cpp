// GaussiansBuffer::decompose<SH>, GaussianPod::decompose<SH> and cov3d_decompose (include/gs3d.hpp) through the C ABI: a grid
// of Gaussians is uploaded as SH f16 / cov f16, which cannot be exported (LossyConfigError); decomposed on the device, with and
// without a selection and to another SH config, it equals the host decomposition of the same records byte for byte, and
// export_ply of the result succeeds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gs3d.hpp"

using namespace gs3d;
#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    // the host function alone: a diagonal covariance gives the identity and the square roots
    const float diag[6] = {4.0f, 0.0f, 0.0f, 0.25f, 0.0f, 9.0f};
    float q[4], sc[3];
    cov3d_decompose(diag, q, sc);
    REQUIRE(q[0] == 0.0f && q[1] == 0.0f && q[2] == 0.0f && q[3] == 1.0f && sc[0] == 2.0f && sc[1] == 0.5f && sc[2] == 3.0f);

    Device dev(0);
    Stream s(dev);
    using Small = GaussianPodWithShHalfCov3dHalfConfigs;
    using Out = GaussianPodWithShHalfCov3dRotScaleConfigs;
    using OutNorm8 = GaussianPodWithShNorm8Cov3dRotScaleConfigs;
    const uint32_t n = 5003;        // four full 1024-blocks and a partial one; not a multiple of 32
    std::vector<Gaussian> all;
    for (uint32_t i = 0; i < n; i++) {
        Gaussian g{};
        const float a = 0.37f * (float)(i % 17), b = 0.11f * (float)(i % 29);
        g.rot[0] = std::sin(a) * std::cos(b); g.rot[1] = std::sin(a) * std::sin(b); g.rot[2] = 0.0f; g.rot[3] = std::cos(a);
        g.pos[0] = ((float)(i % 50) - 24.5f) * 0.125f;
        g.pos[1] = ((float)(i / 50) - 24.5f) * 0.0625f;
        g.pos[2] = -5.0f - (float)(i % 7) * 0.25f;
        g.color[0] = (uint8_t)(i * 37u); g.color[1] = (uint8_t)(i * 11u); g.color[2] = 200; g.color[3] = (uint8_t)(i * 7u);
        for (int k = 0; k < 45; k++) g.sh[k] = 0.001f * (float)((i * 13u + (uint32_t)k * 7u) % 2001u) - 1.0f;
        g.scale[0] = 0.03f; g.scale[1] = i % 4 == 0 ? 0.03f : 0.02f; g.scale[2] = 0.01f + 0.001f * (float)(i % 3);
        all.push_back(g);
    }
    GaussiansBuffer<Small> small(dev, all);
    const std::vector<uint8_t> pods = small.download(s);
    const size_t nb = Small::size(), ob = Out::size();

    // everything, and to another SH config
    const std::vector<uint8_t> want = Small::decompose(pods);
    REQUIRE(want.size() == n * ob);
    GaussiansBuffer<Out> dec = small.decompose(s);
    REQUIRE(dec.len() == n && dec.download(s) == want);
    REQUIRE(small.decompose<GS_SH_NORM8>(s).download(s) == Small::decompose<GS_SH_NORM8>(pods));
    REQUIRE(Small::decompose<GS_SH_NORM8>(pods).size() == n * OutNorm8::size());

    // every third Gaussian, and the others
    Selection sel(dev, n);
    std::vector<uint32_t> words(sel.words(), 0u);
    for (uint32_t i = 0; i < n; i += 3) words[i >> 5] |= 1u << (i & 31u);
    sel.upload(s, words);
    std::vector<uint8_t> third, rest;
    for (uint32_t i = 0; i < n; i++) {
        std::vector<uint8_t> &to = i % 3 == 0 ? third : rest;
        to.insert(to.end(), pods.begin() + i * nb, pods.begin() + (i + 1) * nb);
    }
    REQUIRE(small.decompose(s, &sel).download(s) == Small::decompose(third));
    REQUIRE(small.decompose(s, &sel, true).download(s) == Small::decompose(rest));

    // a rotation + scale source: convert
    REQUIRE(dec.decompose<GS_SH_NORM8>(s, &sel).download(s) == dec.convert<OutNorm8>(s, &sel).download(s));

    // the covariance layout cannot be exported, its decomposition can
    uint64_t count = 0;
    try { check(gs_gaussians_buffer_export_ply(small.raw(), s.raw(), nullptr, 0, nullptr, 0, &count)); REQUIRE(false); } catch (const LossyConfigError &) {}
    check(gs_gaussians_buffer_export_ply(dec.raw(), s.raw(), nullptr, 0, nullptr, 0, &count));
    REQUIRE(count == n);
    std::vector<PlyGaussianPod> ply(n);
    check(gs_gaussians_buffer_export_ply(dec.raw(), s.raw(), nullptr, 0, ply.data(), ply.size(), &count));
    const std::vector<Gaussian> back = Out::into_gaussians(want);
    std::vector<PlyGaussianPod> host(n);
    gs_gaussian_to_ply(back.data(), back.size(), host.data());
    REQUIRE(count == n && std::memcmp(ply.data(), host.data(), n * sizeof(PlyGaussianPod)) == 0);
    REQUIRE(small.download(s) == pods);

    std::printf("cpp decompose OK\n");
    return 0;
}
