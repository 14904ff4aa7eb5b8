// GaussiansBuffer::convert, the concat overload that converts its sources, and the lossy error (include/gs3d.hpp) through the
// C ABI: a grid of Gaussians is uploaded as SH f32 / rot-scale, converted to SH f16 / cov f16 with and without a selection
// and compared with a direct upload in that layout (gs_pack is bit-defined: the same Gaussians give the same pods), then
// merged with a buffer of another layout.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gs3d.hpp"

using namespace gs3d;
#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    Device dev(0);
    Stream s(dev);
    using Full = GaussianPodWithShSingleCov3dRotScaleConfigs;
    using Small = GaussianPodWithShHalfCov3dHalfConfigs;
    using NoSh = GaussianPodWithShNoneCov3dSingleConfigs;
    const uint32_t n = 5003;        // four full 1024-blocks and a partial one; not a multiple of 32
    std::vector<Gaussian> all;
    for (uint32_t i = 0; i < n; i++) {
        Gaussian g{};
        g.rot[0] = 0.1f * (float)(i % 5); g.rot[3] = 1.0f;
        g.pos[0] = ((float)(i % 50) - 24.5f) * 0.125f;
        g.pos[1] = ((float)(i / 50) - 24.5f) * 0.0625f;
        g.pos[2] = -5.0f - (float)(i % 7) * 0.25f;
        g.color[0] = (uint8_t)(i * 37u); g.color[1] = (uint8_t)(i * 11u); g.color[2] = 200; g.color[3] = (uint8_t)(i * 7u);
        for (int k = 0; k < 45; k++) g.sh[k] = 0.001f * (float)((i * 13u + (uint32_t)k * 7u) % 2001u) - 1.0f;
        g.scale[0] = 0.03f; g.scale[1] = 0.02f; g.scale[2] = 0.01f + 0.001f * (float)(i % 3);
        all.push_back(g);
    }
    GaussiansBuffer<Full> full(dev, all);
    GaussiansBuffer<Small> direct(dev, all);
    const std::vector<uint8_t> want = direct.download(s);
    const size_t nb = Small::size();

    // everything
    GaussiansBuffer<Small> conv = full.convert<Small>(s);
    REQUIRE(conv.len() == n);
    REQUIRE(conv.download(s) == want);

    // every third Gaussian, and the others
    Selection sel(dev, n);
    std::vector<uint32_t> words(sel.words(), 0u);
    for (uint32_t i = 0; i < n; i += 3) words[i >> 5] |= 1u << (i & 31u);
    sel.upload(s, words);
    std::vector<uint8_t> third, rest;
    for (uint32_t i = 0; i < n; i++) {
        std::vector<uint8_t> &to = i % 3 == 0 ? third : rest;
        to.insert(to.end(), want.begin() + i * nb, want.begin() + (i + 1) * nb);
    }
    GaussiansBuffer<Small> a = full.convert<Small>(s, &sel), b = full.convert<Small>(s, &sel, true);
    REQUIRE(a.download(s) == third && b.download(s) == rest);

    // identical layouts: extract
    REQUIRE(full.convert<Full>(s, &sel).download(s) == full.extract(s, &sel).download(s));

    // sources of two layouts merged into a third: each part is what convert gives
    GaussiansBuffer<NoSh> nosh = full.convert<NoSh>(s);
    std::vector<uint64_t> counts;
    GaussiansBuffer<Small> merged = GaussiansBuffer<Small>::concat(s, converted, {full.raw(), nosh.raw(), conv.raw()}, {&sel, nullptr, nullptr}, &counts);
    REQUIRE(counts.size() == 3 && counts[0] == third.size() / nb && counts[1] == n && counts[2] == n);
    const std::vector<uint8_t> m = merged.download(s), part1 = nosh.convert<Small>(s).download(s);
    REQUIRE(m.size() == third.size() + 2 * want.size());
    REQUIRE(std::memcmp(m.data(), third.data(), third.size()) == 0);
    REQUIRE(std::memcmp(m.data() + third.size(), part1.data(), part1.size()) == 0);
    REQUIRE(std::memcmp(m.data() + third.size() + part1.size(), want.data(), want.size()) == 0);

    // a covariance does not go back to rotation and scale
    REQUIRE(gs_layout_convertible(Full::sh, Full::cov3d, Small::sh, Small::cov3d) == 1);
    REQUIRE(gs_layout_convertible(Small::sh, Small::cov3d, Full::sh, Full::cov3d) == 0);
    try { conv.convert<Full>(s); REQUIRE(false); } catch (const LossyConfigError &) {}
    try { GaussiansBuffer<Full>::concat(s, converted, {full.raw(), conv.raw()}); REQUIRE(false); } catch (const LossyConfigError &) {}
    REQUIRE(conv.download(s) == want);

    std::printf("cpp convert OK\n");
    return 0;
}
