// GaussiansBuffer::knn, Selection::select_knn and knn_summary (include/gs3d.hpp) through the C ABI: the rows of a jittered
// grid of 1 500 Gaussians with a clump of duplicates, a far outlier and a NaN row against a host double loop with the same
// binary32 operations.  The transform is the default one and the positions are small, so pw = p exactly.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

#include "gs3d.hpp"

using namespace gs3d;
#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static uint32_t bits_of(float v) { uint32_t u; std::memcpy(&u, &v, 4); return u; }

int main() {
    Device dev(0);
    Stream s(dev);
    using G = GaussianPodWithShSingleCov3dRotScaleConfigs;
    const uint32_t n = 1500, k = 5;
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

    // the rows by the definition: candidates within r ordered by (bits of d2, index), the first k, padded
    const float r = 0.3f, rr = r * r;
    std::vector<uint32_t> want_d((size_t)n * k, bits_of(INFINITY)), want_i((size_t)n * k, GS_KNN_NONE);
    uint64_t complete = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (i == 7) {
            for (uint32_t t = 0; t < k; t++) want_d[(size_t)i * k + t] = 0x7fc00000u;
            continue;
        }
        std::vector<std::pair<uint32_t, uint32_t>> cand;
        for (uint32_t j = 0; j < n; j++) {
            if (j == i || j == 7) continue;
            const volatile float dx = all[i].pos[0] - all[j].pos[0], dy = all[i].pos[1] - all[j].pos[1], dz = all[i].pos[2] - all[j].pos[2];
            const volatile float xx = dx * dx, yy = dy * dy, zz = dz * dz;      // (volatile: every product and sum rounded to binary32)
            const volatile float xy = xx + yy;
            const volatile float d2 = xy + zz;
            if (d2 <= rr) cand.push_back({bits_of(d2), j});
        }
        std::sort(cand.begin(), cand.end());
        for (uint32_t t = 0; t < k && t < cand.size(); t++) {
            want_d[(size_t)i * k + t] = cand[t].first;
            want_i[(size_t)i * k + t] = cand[t].second;
        }
        complete += cand.size() >= k ? 1 : 0;
    }
    Buffer dist2(dev, (size_t)n * k * 4), index(dev, (size_t)n * k * 4);
    buf.knn(s, k, r, dist2, &index);
    const std::vector<uint32_t> got_d = dist2.download<uint32_t>(s), got_i = index.download<uint32_t>(s);
    REQUIRE(got_d.size() == (size_t)n * k && got_i.size() == (size_t)n * k);
    REQUIRE(got_d == want_d);
    REQUIRE(got_i == want_i);
    REQUIRE(got_i[8 * k] == GS_KNN_NONE && got_d[8 * k] == bits_of(INFINITY));            // the far outlier: nobody within r
    REQUIRE(got_d[1400 * k + k - 1] == 0u && got_i[1400 * k] == 1401u && got_i[1401 * k] == 1400u);      // the clump: ties by index
    REQUIRE(complete > 0 && complete < n - 1);

    // without the index plane, and only the rows of a query selection: the others keep their bytes
    Buffer again(dev, (size_t)n * k * 4);
    Selection queries(dev, n);
    queries.select_range(s, 100, 50);
    buf.knn(s, k, 2.0f * r, again);
    buf.knn(s, k, r, again, nullptr, nullptr, &queries);
    const std::vector<uint32_t> mixed = again.download<uint32_t>(s);
    buf.knn(s, k, 2.0f * r, again);
    const std::vector<uint32_t> wide = again.download<uint32_t>(s);
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t t = 0; t < k; t++) REQUIRE(mixed[(size_t)i * k + t] == (i >= 100 && i < 150 ? want_d : wide)[(size_t)i * k + t]);

    // the incomplete rows: v = +inf; the NaN row is never selected
    Selection sel(dev, n);
    sel.select_knn(s, dist2, k, GS_KNN_KTH_DIST2, INFINITY, INFINITY);
    const std::vector<uint32_t> words = sel.download(s);
    for (uint32_t i = 0; i < n; i++) {
        const bool bit = (words[i >> 5] >> (i & 31u)) & 1u;
        REQUIRE(bit == (i != 7 && want_d[(size_t)i * k + k - 1] == bits_of(INFINITY)));
    }
    REQUIRE(sel.count(s) == n - 1 - complete);

    // the summary of the mean distance against the same arithmetic on the host
    double sum = 0.0, sum_sq = 0.0;
    uint32_t mn = bits_of(INFINITY), mx = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (i == 7 || want_d[(size_t)i * k + k - 1] == bits_of(INFINITY)) continue;
        volatile float acc = 0.0f;
        for (uint32_t t = 0; t < k; t++) {
            float d;
            std::memcpy(&d, &want_d[(size_t)i * k + t], 4);
            const volatile float root = std::sqrt(d);
            acc = t ? acc + root : root;
        }
        const volatile float v = acc / (float)k;
        sum += (double)v;
        sum_sq += (double)v * (double)v;
        mn = std::min(mn, bits_of(v));
        mx = std::max(mx, bits_of(v));
    }
    const gs_knn_summary_result m = knn_summary(s, dist2, n, k, GS_KNN_MEAN_DIST);
    REQUIRE(m.points == n - 1 && m.complete == complete);
    REQUIRE(bits_of(m.min) == mn && bits_of(m.max) == mx);
    REQUIRE(std::fabs(m.sum - sum) <= (double)complete * 0x1p-52 * sum && std::fabs(m.sum_sq - sum_sq) <= (double)complete * 0x1p-52 * sum_sq);
    const gs_knn_summary_result kth = knn_summary(s, dist2, n, k, GS_KNN_KTH_DIST2);
    REQUIRE(kth.complete == complete && kth.min == 0.0f && kth.max <= rr);

    try { buf.knn(s, 0, r, dist2); REQUIRE(false); } catch (const Error &) {}
    try { buf.knn(s, 17, r, dist2); REQUIRE(false); } catch (const Error &) {}
    try { sel.select_knn(s, dist2, k, 2, 0.0f, 1.0f); REQUIRE(false); } catch (const Error &) {}
    try { (void)knn_summary(s, dist2, n + 1, k, GS_KNN_MEAN_DIST); REQUIRE(false); } catch (const Error &) {}
    REQUIRE(sel.count(s) == n - 1 - complete);
    REQUIRE(dist2.download<uint32_t>(s) == want_d);
    std::printf("cpp knn OK\n");
    return 0;
}
