// GaussiansBuffer::knn_to, GaussiansBuffer::pair_sums, rigid_fit and compose (include/gs3d.hpp) through the C ABI: the rows of
// 700 queries against a jittered grid of 1 200 targets with a clump of duplicates, a far outlier and a NaN on each side,
// against a host double loop with the same binary32 operations; then one ICP step on a moved copy of part of the target.
// The transforms are the default one and the positions are small, so pw = p exactly.
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
    using T = GaussianPodWithShNoneCov3dSingleConfigs;
    const uint32_t nt = 1200, nq = 700, k = 4;
    uint32_t seed = 4242u;
    auto jitter = [&seed]() { seed = seed * 1664525u + 1013904223u; return (float)(seed >> 20) * (1.0f / 4096.0f) - 0.5f; };
    auto make = [](float x, float y, float z) {
        Gaussian g{};
        g.rot[3] = 1.0f;
        g.pos[0] = x; g.pos[1] = y; g.pos[2] = z;
        g.scale[0] = g.scale[1] = g.scale[2] = 0.01f;
        g.color[3] = 255;
        return g;
    };
    std::vector<Gaussian> target, query;
    for (uint32_t i = 0; i < nt; i++)
        target.push_back(make(((float)(i % 10) + 0.2f * jitter()) * 0.25f, ((float)((i / 10) % 10) + 0.2f * jitter()) * 0.25f,
                              -4.0f + ((float)(i / 100) + 0.2f * jitter()) * 0.25f));
    for (uint32_t i = 1100; i < 1180; i++) { target[i].pos[0] = 1.0f; target[i].pos[1] = 1.0f; target[i].pos[2] = -3.0f; }      // 80 duplicates
    // the queries: a rotation of 1.5 degrees about z through (1.1, 1.1) and a small shift of every second target of the first
    // 1 400 / 2; then a duplicate of the clump, a NaN and two queries outside the target's box
    const float c = std::cos(0.026f), sn = std::sin(0.026f);
    for (uint32_t i = 0; i < nq; i++) {
        const Gaussian &m = target[(2 * i) % 1100 + (2 * i >= 1100 ? 1 : 0)];
        const float x = m.pos[0] - 1.1f, y = m.pos[1] - 1.1f;
        query.push_back(make(1.1f + c * x - sn * y + 0.01f, 1.1f + sn * x + c * y - 0.015f, m.pos[2] + 0.02f));
    }
    target[307].pos[1] = NAN;      // (307 and 309 are the mates of no query)
    target[309].pos[0] = target[309].pos[1] = target[309].pos[2] = 1.0e6f;
    query[3] = make(1.0f, 1.0f, -3.0f);
    query[5].pos[2] = NAN;
    query[6] = make(-0.1f, 1.0f, -3.5f);
    query[9] = make(50.0f, 1.0f, -3.5f);
    GaussiansBuffer<G> qbuf(dev, query);
    GaussiansBuffer<T> tbuf(dev, target);

    // the rows by the definition: target points within r ordered by (bits of d2, target index), the first k, padded
    const float r = 0.3f, rr = r * r;
    std::vector<uint32_t> want_d((size_t)nq * k, bits_of(INFINITY)), want_i((size_t)nq * k, GS_KNN_NONE);
    uint64_t with_neighbour = 0;
    for (uint32_t i = 0; i < nq; i++) {
        if (i == 5) {
            for (uint32_t t = 0; t < k; t++) want_d[(size_t)i * k + t] = 0x7fc00000u;
            continue;
        }
        std::vector<std::pair<uint32_t, uint32_t>> cand;
        for (uint32_t j = 0; j < nt; j++) {
            if (j == 307) continue;
            const volatile float dx = query[i].pos[0] - target[j].pos[0], dy = query[i].pos[1] - target[j].pos[1], dz = query[i].pos[2] - target[j].pos[2];
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
        with_neighbour += cand.empty() ? 0 : 1;
    }
    Buffer dist2(dev, (size_t)nq * k * 4), index(dev, (size_t)nq * k * 4);
    qbuf.knn_to(s, tbuf, k, r, dist2, &index);
    const std::vector<uint32_t> got_d = dist2.download<uint32_t>(s), got_i = index.download<uint32_t>(s);
    REQUIRE(got_d.size() == (size_t)nq * k && got_i.size() == (size_t)nq * k);
    for (size_t e = 0; e < got_d.size(); e++)
        if (got_d[e] != want_d[e] || got_i[e] != want_i[e]) {
            std::printf("row %zu entry %zu: d2 %08x index %u, want %08x %u\n", e / k, e % k, got_d[e], got_i[e], want_d[e], want_i[e]);
            break;
        }
    REQUIRE(got_d == want_d);
    REQUIRE(got_i == want_i);
    REQUIRE(got_d[3 * k + k - 1] == 0u && got_i[3 * k] == 1100u && got_i[3 * k + 3] == 1103u);      // the clump: ties by target index
    REQUIRE(got_i[9 * k] == GS_KNN_NONE && got_d[9 * k] == bits_of(INFINITY));                      // far outside the box
    REQUIRE(got_i[6 * k] != GS_KNN_NONE);                                                           // outside the box, within r of it

    // only the rows of a query selection, without the index plane: the others keep their bytes
    Buffer again(dev, (size_t)nq * k * 4);
    Selection queries(dev, nq);
    queries.select_range(s, 100, 50);
    qbuf.knn_to(s, tbuf, k, 2.0f * r, again);
    qbuf.knn_to(s, tbuf, k, r, again, nullptr, &queries);
    const std::vector<uint32_t> mixed = again.download<uint32_t>(s);
    qbuf.knn_to(s, tbuf, k, 2.0f * r, again);
    const std::vector<uint32_t> wide = again.download<uint32_t>(s);
    for (uint32_t i = 0; i < nq; i++)
        for (uint32_t t = 0; t < k; t++) REQUIRE(mixed[(size_t)i * k + t] == (i >= 100 && i < 150 ? want_d : wide)[(size_t)i * k + t]);

    // the overlap: the plane is a k-NN plane, select_knn takes it unchanged
    Selection near(dev, nq);
    Buffer first(dev, (size_t)nq * 4), first_i(dev, (size_t)nq * 4);
    qbuf.knn_to(s, tbuf, 1, r, first, &first_i);
    near.select_knn(s, first, 1, GS_KNN_KTH_DIST2, 0.0f, rr);
    REQUIRE(near.count(s) == with_neighbour);

    // the pair sums of the nearest neighbours against a host loop in the same order of operations per pair
    const std::vector<uint32_t> mate = first_i.download<uint32_t>(s);
    double want[18] = {0}, want_abs[18] = {0};
    uint64_t pairs = 0;
    for (uint32_t i = 0; i < nq; i++) {
        REQUIRE(mate[i] == want_i[(size_t)i * k]);
        if (mate[i] >= nt || i == 5) continue;
        const double p[3] = {query[i].pos[0], query[i].pos[1], query[i].pos[2]};
        const double q[3] = {target[mate[i]].pos[0], target[mate[i]].pos[1], target[mate[i]].pos[2]};
        pairs++;
        for (int a = 0; a < 3; a++) {
            want[a] += p[a];
            want[3 + a] += q[a];
            for (int b = 0; b < 3; b++) want[6 + 3 * a + b] += p[a] * q[b];
        }
        want[15] += (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2];
        want[16] += (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2];
        want[17] += ((p[0] - q[0]) * (p[0] - q[0]) + (p[1] - q[1]) * (p[1] - q[1])) + (p[2] - q[2]) * (p[2] - q[2]);
        for (int a = 0; a < 3; a++) {
            want_abs[a] += std::fabs(p[a]);
            want_abs[3 + a] += std::fabs(q[a]);
            for (int b = 0; b < 3; b++) want_abs[6 + 3 * a + b] += std::fabs(p[a] * q[b]);
        }
    }
    for (int f = 15; f < 18; f++) want_abs[f] = want[f];      // sums of squares
    const gs_pair_sums sums = qbuf.pair_sums(s, tbuf, first_i), twice = qbuf.pair_sums(s, tbuf, first_i);
    REQUIRE(sums.pairs == pairs && pairs == with_neighbour);
    REQUIRE(std::memcmp(&sums, &twice, sizeof(sums)) == 0 && sizeof(sums) == 152);
    double got[18];      // sp, sq, spq, spp, sqq, sdd lie behind the count
    std::memcpy(got, (const char *)&sums + 8, sizeof(got));
    // both sides add `pairs` values in some order: twice the first-order bound of one summation
    for (int f = 0; f < 18; f++) REQUIRE(std::fabs(got[f] - want[f]) <= (double)pairs * 0x1p-52 * want_abs[f]);

    // one ICP step: the fit removes the rigid part; what is left is the pair of the query outside the box (0.13 of 700 pairs)
    double rms = 0.0;
    const gs_model_transform_pod delta = rigid_fit(sums, false, &rms);
    REQUIRE(rms > 0.02 && rms < 0.2 && delta.scale[0] == 1.0f && delta.rot[3] > 0.99f);
    REQUIRE(std::fabs(delta.rot[2] + std::sin(0.013f)) < 2e-3 && std::fabs(delta.rot[0]) < 2e-3 && std::fabs(delta.rot[1]) < 2e-3);
    gs_model_transform_pod ident;
    gs_model_transform_pod_default(&ident);
    const gs_model_transform_pod moved = compose(delta, ident);
    REQUIRE(std::memcmp(moved.pos, delta.pos, 12) == 0 && std::memcmp(moved.rot, delta.rot, 16) == 0);
    qbuf.knn_to(s, tbuf, 1, r, first, &first_i, nullptr, nullptr, &moved);
    const gs_pair_sums after = qbuf.pair_sums(s, tbuf, first_i, 1, nullptr, &moved);
    REQUIRE(after.pairs >= pairs && std::sqrt(after.sdd / (double)after.pairs) < 0.5 * rms);

    // an index plane of values >= nt names no pair
    std::vector<uint32_t> none(nq, GS_KNN_NONE);
    Buffer poisoned(dev, (size_t)nq * 4, none.data());
    REQUIRE(qbuf.pair_sums(s, tbuf, poisoned).pairs == 0);

    try { qbuf.knn_to(s, tbuf, 0, r, dist2); REQUIRE(false); } catch (const Error &) {}
    try { qbuf.knn_to(s, tbuf, 17, r, dist2); REQUIRE(false); } catch (const Error &) {}
    try { qbuf.knn_to(s, qbuf, k, r, dist2); REQUIRE(false); } catch (const Error &) {}
    try { qbuf.knn_to(s, tbuf, k, -1.0f, dist2); REQUIRE(false); } catch (const Error &) {}
    try { gs_pair_sums two = sums; two.pairs = 2; (void)rigid_fit(two); REQUIRE(false); } catch (const Error &) {}
    REQUIRE(dist2.download<uint32_t>(s) == want_d);
    std::printf("cpp align OK\n");
    return 0;
}
