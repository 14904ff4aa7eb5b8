// GaussiansBuffer::neighbor_counts and Selection::select_neighbors (include/gs3d.hpp) through the C ABI: the counts of a
// jittered grid of 1 500 Gaussians with a clump, a far outlier and a NaN row against a host double loop with the same
// binary32 operations.  The transform is the default one and the positions are small, so pw = p exactly.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gs3d.hpp"

using namespace gs3d;
#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
    Device dev(0);
    Stream s(dev);
    using G = GaussianPodWithShSingleCov3dRotScaleConfigs;
    const uint32_t n = 1500;
    std::vector<Gaussian> all;
    uint32_t seed = 12345u;
    auto jitter = [&seed]() { seed = seed * 1664525u + 1013904223u; return (float)(seed >> 20) * (1.0f / 4096.0f) - 0.5f; };
    for (uint32_t i = 0; i < n; i++) {
        Gaussian g{};
        g.rot[3] = 1.0f;
        g.pos[0] = ((float)(i % 12) + 0.75f * jitter()) * 0.25f;
        g.pos[1] = ((float)((i / 12) % 12) + 0.75f * jitter()) * 0.25f;
        g.pos[2] = -4.0f + ((float)(i / 144) + 0.75f * jitter()) * 0.25f;
        if (i >= 1400 && i < 1440) { g.pos[0] = 1.0f; g.pos[1] = 1.0f; g.pos[2] = -3.0f; }      // 40 duplicates
        g.scale[0] = g.scale[1] = g.scale[2] = 0.01f;
        g.color[3] = 255;
        all.push_back(g);
    }
    all[7].pos[1] = NAN;
    all[8].pos[0] = 1.0e6f; all[8].pos[1] = 1.0e6f; all[8].pos[2] = 1.0e6f;
    GaussiansBuffer<G> buf(dev, all);

    const float r = 0.3f, rr = r * r;
    std::vector<uint32_t> want(n, 0u);
    for (uint32_t i = 0; i < n; i++) {
        if (i == 7) continue;
        for (uint32_t j = 0; j < n; j++) {
            if (j == i || j == 7) continue;
            const volatile float dx = all[i].pos[0] - all[j].pos[0], dy = all[i].pos[1] - all[j].pos[1], dz = all[i].pos[2] - all[j].pos[2];
            const volatile float xx = dx * dx, yy = dy * dy, zz = dz * dz;      // (volatile: every product and sum rounded to binary32)
            const volatile float xy = xx + yy;
            const volatile float d2 = xy + zz;
            want[i] += d2 <= rr ? 1u : 0u;
        }
    }
    Buffer plane(dev, (size_t)n * 4);
    buf.neighbor_counts(s, r, UINT32_MAX, plane);
    const std::vector<uint32_t> got = plane.download<uint32_t>(s);
    REQUIRE(got.size() == n);
    REQUIRE(got == want);
    REQUIRE(got[7] == 0 && got[8] == 0 && got[1400] >= 39);

    buf.neighbor_counts(s, r, 5, plane);
    const std::vector<uint32_t> capped = plane.download<uint32_t>(s);
    for (uint32_t i = 0; i < n; i++) REQUIRE(capped[i] == (want[i] < 5u ? want[i] : 5u));

    // the floaters: fewer than 3 others around; the NaN row is never selected
    Selection sel(dev, n);
    sel.select_neighbors(s, buf, r, 0, 2);
    const std::vector<uint32_t> words = sel.download(s);
    uint64_t floaters = 0;
    for (uint32_t i = 0; i < n; i++) {
        const bool bit = (words[i >> 5] >> (i & 31u)) & 1u;
        REQUIRE(bit == (i != 7 && want[i] <= 2u));
        floaters += bit ? 1 : 0;
    }
    REQUIRE(floaters > 0 && sel.count(s) == floaters);
    try { sel.select_neighbors(s, buf, -1.0f); REQUIRE(false); } catch (const Error &) {}
    try { buf.neighbor_counts(s, r, 0, plane); REQUIRE(false); } catch (const Error &) {}
    REQUIRE(sel.count(s) == floaters);
    std::printf("cpp neighbors OK\n");
    return 0;
}
