// GaussiansBuffer::components, Selection::select_components and Selection::select_connected (include/gs3d.hpp) through the
// C ABI: labels, sizes, info and both selects of a jittered grid of 1 500 Gaussians with a clump of duplicates, a detached
// floater clump, a far outlier and a NaN row against a host union-find over a double loop with the same binary32
// operations.  The transform is the default one and the positions are small, so pw = p exactly.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>

#include "gs3d.hpp"

using namespace gs3d;
#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static uint32_t find(std::vector<uint32_t> &p, uint32_t x) {
    while (p[x] != x) x = p[x] = p[p[x]];
    return x;
}

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
        if (i >= 1440 && i < 1470) { g.pos[0] = 9.0f + 0.1f * jitter(); g.pos[1] = 0.1f * jitter(); g.pos[2] = 0.1f * jitter(); }   // a clump of 30
        g.scale[0] = g.scale[1] = g.scale[2] = 0.01f;
        g.color[3] = 255;
        all.push_back(g);
    }
    all[7].pos[1] = NAN;
    all[8].pos[0] = 1.0e6f; all[8].pos[1] = 1.0e6f; all[8].pos[2] = 1.0e6f;
    GaussiansBuffer<G> buf(dev, all);

    const float r = 0.24f, rr = r * r;
    std::vector<uint32_t> parent(n);
    std::iota(parent.begin(), parent.end(), 0u);
    for (uint32_t i = 0; i < n; i++) {
        if (i == 7) continue;
        for (uint32_t j = 0; j < i; j++) {
            if (j == 7) continue;
            const volatile float dx = all[i].pos[0] - all[j].pos[0], dy = all[i].pos[1] - all[j].pos[1], dz = all[i].pos[2] - all[j].pos[2];
            const volatile float xx = dx * dx, yy = dy * dy, zz = dz * dz;      // (volatile: every product and sum rounded to binary32)
            const volatile float xy = xx + yy;
            const volatile float d2 = xy + zz;
            if (d2 <= rr) {
                const uint32_t a = find(parent, i), b = find(parent, j);
                if (a != b) parent[a > b ? a : b] = a > b ? b : a;      // the smaller index stays the root: the label
            }
        }
    }
    std::vector<uint32_t> want_l(n), want_s(n, 0u), members(n, 0u);
    for (uint32_t i = 0; i < n; i++)
        if (i != 7) members[find(parent, i)]++;
    gs_components_info want{};
    want.largest_label = GS_COMPONENT_NONE;
    for (uint32_t i = 0; i < n; i++) {
        want_l[i] = i == 7 ? GS_COMPONENT_NONE : find(parent, i);
        want_s[i] = i == 7 ? 0u : members[want_l[i]];
        want.points += i != 7;
        want.components += want_l[i] == i;
    }
    for (uint32_t i = 0; i < n; i++)
        if (want_l[i] == i && want_s[i] > want.largest) { want.largest = want_s[i]; want.largest_label = i; }

    Buffer labels(dev, (size_t)n * 4), sizes(dev, (size_t)n * 4), info(dev, sizeof(gs_components_info));
    buf.components(s, r, &labels, &sizes, &info);
    const std::vector<uint32_t> got_l = labels.download<uint32_t>(s), got_s = sizes.download<uint32_t>(s);
    const std::vector<uint32_t> got_i = info.download<uint32_t>(s);
    REQUIRE(got_l == want_l);
    REQUIRE(got_s == want_s);
    REQUIRE(got_i.size() == 4 && got_i[0] == want.points && got_i[1] == want.components && got_i[2] == want.largest &&
            got_i[3] == want.largest_label);
    REQUIRE(got_l[7] == GS_COMPONENT_NONE && got_s[7] == 0 && got_l[8] == 8 && got_s[8] == 1);
    REQUIRE(got_s[1400] >= 40 && got_l[1439] == got_l[1400]);
    REQUIRE(got_l[1469] == 1440 && got_s[1440] == 30);                        // the clump is one cluster of 30
    REQUIRE(want.components > 3 && want.largest > 100);
    // only the sizes, only the info
    buf.components(s, r, nullptr, &sizes, nullptr);
    REQUIRE(sizes.download<uint32_t>(s) == want_s);
    buf.components(s, r, nullptr, nullptr, &info);
    REQUIRE(info.download<uint32_t>(s) == got_i);

    // remove small clusters: everything smaller than 50; the NaN row is never selected
    Selection sel(dev, n);
    sel.select_components(s, buf, r, 0, 49);
    std::vector<uint32_t> words = sel.download(s);
    uint64_t small = 0;
    for (uint32_t i = 0; i < n; i++) {
        const bool bit = (words[i >> 5] >> (i & 31u)) & 1u;
        REQUIRE(bit == (i != 7 && want_s[i] <= 49u));
        small += bit ? 1 : 0;
    }
    REQUIRE(small >= 71 && small < n && sel.count(s) == small);
    // select all of what was picked: one Gaussian of the clump, one of the NaN row
    Selection seeds(dev, n);
    seeds.select_range(s, 1450, 1);
    seeds.select_range(s, 7, 1, GS_SEL_OR);
    sel.select_connected(s, buf, r, seeds);
    words = sel.download(s);
    for (uint32_t i = 0; i < n; i++) REQUIRE((bool)((words[i >> 5] >> (i & 31u)) & 1u) == (i >= 1440 && i < 1470));
    // ... and grown in place
    seeds.select_connected(s, buf, r, seeds);
    REQUIRE(seeds.download(s) == words && seeds.count(s) == 30);
    try { sel.select_components(s, buf, -1.0f); REQUIRE(false); } catch (const Error &) {}
    try { buf.components(s, r, nullptr, nullptr, nullptr); REQUIRE(false); } catch (const Error &) {}
    REQUIRE(sel.count(s) == 30);
    std::printf("cpp components OK\n");
    return 0;
}
