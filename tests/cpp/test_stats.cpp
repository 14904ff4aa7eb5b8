// GaussiansBuffer::stats / histogram and Selection::select_attribute (include/gs3d.hpp) through the C ABI: the statistics
// and one histogram of a grid of 5 003 Gaussians against a host loop over the same records.  The positions are small
// dyadic numbers and the transform is the default one, so the host loop's world positions are exact.
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
    const uint32_t n = 5003;        // four full 1024-blocks and a partial one; not a multiple of 32
    std::vector<Gaussian> all;
    for (uint32_t i = 0; i < n; i++) {
        Gaussian g{};
        g.rot[3] = 1.0f;
        g.pos[0] = ((float)(i % 50) - 24.5f) * 0.125f;
        g.pos[1] = ((float)(i / 50) - 24.5f) * 0.0625f;
        g.pos[2] = -5.0f - (float)(i % 7) * 0.25f;
        g.color[0] = (uint8_t)(i * 37u); g.color[1] = (uint8_t)(i * 11u); g.color[2] = 200; g.color[3] = (uint8_t)(i * 7u);
        g.scale[0] = 0.03f; g.scale[1] = 0.02f; g.scale[2] = 0.01f;
        all.push_back(g);
    }
    GaussiansBuffer<G> buf(dev, all);

    // every third Gaussian
    Selection sel(dev, n);
    std::vector<uint32_t> words(sel.words(), 0u);
    for (uint32_t i = 0; i < n; i += 3) words[i >> 5] |= 1u << (i & 31u);
    sel.upload(s, words);

    uint64_t count = 0;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    double sum[3] = {0, 0, 0};
    for (uint32_t i = 0; i < n; i += 3, count++)
        for (int k = 0; k < 3; k++) {
            lo[k] = std::fmin(lo[k], all[i].pos[k]);
            hi[k] = std::fmax(hi[k], all[i].pos[k]);
            sum[k] += (double)all[i].pos[k];      // multiples of 2^-4 below 2^10: exact in any order
        }
    const gs_stats st = buf.stats(s, &sel);
    REQUIRE(st.count == count);
    for (int k = 0; k < 3; k++) {
        REQUIRE(st.attr[GS_ATTR_X + k].finite == count);
        REQUIRE(st.attr[GS_ATTR_X + k].min == lo[k] && st.attr[GS_ATTR_X + k].max == hi[k]);
        REQUIRE(st.attr[GS_ATTR_X + k].sum == sum[k]);
    }
    REQUIRE(st.attr[GS_ATTR_BLUE].min == 200.0f / 255.0f && st.attr[GS_ATTR_BLUE].max == 200.0f / 255.0f);
    REQUIRE(st.attr[GS_ATTR_SIZE2].finite == count && st.attr[GS_ATTR_SIZE2].min > 0.0f);
    const gs_stats whole = buf.stats(s);
    REQUIRE(whole.count == n && whole.attr[GS_ATTR_OPACITY].finite == n);

    // opacity in 16 bins over [0.25, 0.75): both rows against the host loop
    gs_attribute_desc a{};
    a.attr = GS_ATTR_OPACITY;
    const uint32_t bins = 16;
    const std::vector<uint64_t> h = buf.histogram(s, a, 0.25f, 0.75f, bins, &sel);
    REQUIRE(h.size() == 2 * (bins + 3));
    std::vector<uint64_t> want(2 * (bins + 3), 0);
    const float scale = (float)bins / (0.75f - 0.25f);
    for (uint32_t i = 0; i < n; i++) {
        const float v = (float)all[i].color[3] / 255.0f;
        uint32_t slot = v < 0.25f ? bins : v >= 0.75f ? bins + 1 : (uint32_t)((v - 0.25f) * scale);
        if (slot < bins && slot > bins - 1) slot = bins - 1;
        want[(i % 3 == 0 ? 0 : bins + 3) + slot]++;
    }
    REQUIRE(h == want);
    uint64_t row0 = 0, row1 = 0;
    for (uint32_t k = 0; k < bins + 3; k++) { row0 += h[k]; row1 += h[bins + 3 + k]; }
    REQUIRE(row0 == count && row1 == n - count && h[bins] > 0 && h[bins + 1] > 0);

    // the cleanup step: the Gaussians of low opacity
    Selection low(dev, n);
    low.select_attribute(s, buf, a, 0.0f, 0.1f);
    uint64_t low_want = 0;
    for (uint32_t i = 0; i < n; i++) low_want += (float)all[i].color[3] / 255.0f <= 0.1f ? 1 : 0;
    REQUIRE(low.count(s) == low_want && low_want > 0);
    a.attr = GS_ATTR_COUNT;
    try { low.select_attribute(s, buf, a, 0.0f, 0.1f); REQUIRE(false); } catch (const Error &) {}
    REQUIRE(low.count(s) == low_want);
    std::printf("cpp stats OK\n");
    return 0;
}
