// gs_knn_kernels.h — the k nearest neighbours of the device editor (include/gs3d.h gs_gaussians_buffer_knn, gs_select_knn,
// gs_knn_summary): for every POINT of §3.11 the k smallest binary32 squared distances to other points within
// a radius, with the caller indices they belong to, ordered by (bits of d2, caller index).  No reference item: the
// reference has no neighbour search.
//
// The row is defined without a grid; the sorted cell grid of §3.11 (gs_neighbor_grid.h, the front of gs_neighbors.hip) only
// bounds the candidates: a cell side is at least r (1 + 2^-10), so every candidate of a query lies in the 27 cells around it.
// Every operation is rounded (-ffp-contract=off).
#pragma once

#include "gs_neighbor_grid.h"

namespace gs {

constexpr uint32_t KNN_MAX_K = 16u;
constexpr uint32_t KNN_NONE = 0xffffffffu;        // GS_KNN_NONE: the index of a padding entry
constexpr uint32_t KNN_INF = 0x7f800000u;         // +inf: the distance of a padding entry
constexpr uint32_t KNN_NAN = 0x7fc00000u;         // every distance of a written row that belongs to no point
// an entry of a row is ONE 64-bit word (bits of d2 << 32) | caller index: d2 >= +0 is never NaN for points, so the unsigned
// order of the words is the order of the definition, ties by index included
constexpr uint64_t KNN_PAD = ((uint64_t)KNN_INF << 32) | KNN_NONE;
enum { KNN_KTH_DIST2 = 0, KNN_MEAN_DIST = 1 };

// The traversal of k_nb_count (gs_neighbor_kernels.h: 64 sorted queries per wave, groups of one row of cells at most NB_SPAN
// cells long, 18 binary searches side by side, the 9 runs streamed 64 candidates at a time and broadcast by v_readlane), with
// these differences.  A lane keeps its K best entries ascending in e[0..K): registers, because every index below is a
// constant after unrolling.  A candidate enters through a compare-exchange chain: x = min / max against e[0], e[1], ... in turn
// leaves e sorted with the largest of the K + 1 dropped.  e starts as K paddings, so "fewer than K held" needs no counter and
// the acceptance bound is rr while the row is incomplete and e[K - 1] once it is complete.  The chain is skipped for the whole
// wave when no lane accepts; the caller index of a candidate (vals[c], loaded with its position) is broadcast only then.
// The query bit of slot s is bit vals[s] of `queries` (null: all); a wave without queries leaves at once.  A query that is no
// point writes a row of NaN / NONE.  dist2[i K + t], index[i K + t]: row i in caller order; index may be null.
template <int K>
__global__ __launch_bounds__(256) void k_nb_knn(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                const float *__restrict__ sx, const float *__restrict__ sy,
                                                const float *__restrict__ sz, uint32_t n, float rr,
                                                const uint32_t *__restrict__ queries, uint32_t *__restrict__ dist2,
                                                uint32_t *__restrict__ index) {
    const uint32_t lane = threadIdx.x & 63u, s = blockIdx.x * 256u + threadIdx.x;
    uint64_t key = NB_KEY_NONE;
    uint32_t self = 0u;
    bool query = false;
    if (s < n) {
        key = keys[s];
        self = vals[s];
        query = queries ? (queries[self >> 5] >> (self & 31u)) & 1u : true;
    }
    if (!__any(query)) return;
    const bool point = key != NB_KEY_NONE;
    const uint32_t qx = (uint32_t)key & NB_CELL_MAX, row_lo = (uint32_t)(key >> NB_CELL_BITS), row_hi = (uint32_t)(key >> (NB_CELL_BITS + 32u));
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    if (point) {
        px = sx[s];
        py = sy[s];
        pz = sz[s];
    }
    uint64_t e[K];
#pragma unroll
    for (int t = 0; t < K; t++) e[t] = KNN_PAD;
    uint64_t todo = __ballot(point && query);
    while (todo) {
        const uint32_t leader = (uint32_t)__builtin_ctzll(todo);
        const uint32_t l_lo = nb_readlane(row_lo, leader), l_hi = nb_readlane(row_hi, leader), l_qx = nb_readlane(qx, leader);
        const bool in = ((todo >> lane) & 1ull) && row_lo == l_lo && row_hi == l_hi && qx - l_qx <= NB_SPAN;
        const uint64_t group = __ballot(in);      // (the leader's bit at least)
        todo &= ~group;
        const uint32_t last_qx = nb_readlane(qx, 63u - (uint32_t)__builtin_clzll(group));
        const uint32_t x0 = l_qx ? l_qx - 1u : 0u, x1 = last_qx < NB_CELL_MAX ? last_qx + 1u : NB_CELL_MAX;
        const uint32_t l_qy = l_lo & NB_CELL_MAX, l_qz = (uint32_t)((((uint64_t)l_hi << 32) | l_lo) >> NB_CELL_BITS);
        // lane 2 k: the first slot of row k with cell x >= x0; lane 2 k + 1: the first slot behind its cells x <= x1
        const uint32_t k9 = lane >> 1;
        const int32_t tz = (int32_t)l_qz + (int32_t)(k9 / 3u) - 1, ty = (int32_t)l_qy + (int32_t)(k9 % 3u) - 1;
        const bool search = lane < 18u && tz >= 0 && tz <= (int32_t)NB_CELL_MAX && ty >= 0 && ty <= (int32_t)NB_CELL_MAX;
        const bool upper = lane & 1u;
        const uint64_t target = ((uint64_t)(uint32_t)tz << (2u * NB_CELL_BITS)) | ((uint64_t)(uint32_t)ty << NB_CELL_BITS) | (upper ? x1 : x0);
        uint32_t lo = 0u, hi = search ? n : 0u;      // (a row outside the grid: the empty run [0, 0))
        while (__any(lo < hi)) {
            if (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2u;
                const uint64_t k = keys[mid];
                if (upper ? k <= target : k < target) lo = mid + 1u;
                else hi = mid;
            }
        }
        for (uint32_t k = 0u; k < 9u; k++) {
            const uint32_t begin = nb_readlane(lo, 2u * k), end = nb_readlane(lo, 2u * k + 1u);
            for (uint32_t t = begin; t < end; t += 64u) {
                const uint32_t c = t + lane, m = end - t < 64u ? end - t : 64u;
                float cx = 0.0f, cy = 0.0f, cz = 0.0f;
                uint32_t cv = 0u;
                if (c < end) {
                    cx = sx[c];
                    cy = sy[c];
                    cz = sz[c];
                    cv = vals[c];
                }
                for (uint32_t j = 0u; j < m; j++) {
                    const float dx = px - nb_readlane_f(cx, j), dy = py - nb_readlane_f(cy, j), dz = pz - nb_readlane_f(cz, j);
                    const float d2 = (dx * dx + dy * dy) + dz * dz;
                    // (the exact test against e[K - 1], index included, is the chain's own first comparison)
                    const bool maybe = in && d2 <= rr && f2u(d2) <= (uint32_t)(e[K - 1] >> 32) && t + j != s;
                    if (__any(maybe)) {
                        uint64_t x = maybe ? ((uint64_t)f2u(d2) << 32) | nb_readlane(cv, j) : ~0ull;
#pragma unroll
                        for (int u = 0; u < K; u++) {
                            const bool less = x < e[u];
                            const uint64_t small = less ? x : e[u];
                            x = less ? e[u] : x;
                            e[u] = small;
                        }
                    }
                }
            }
        }
    }
    if (s < n && query) {
        const uint64_t row = (uint64_t)self * (uint32_t)K;
#pragma unroll
        for (int t = 0; t < K; t++) {
            dist2[row + t] = point ? (uint32_t)(e[t] >> 32) : KNN_NAN;
            if (index) index[row + t] = point ? (uint32_t)e[t] : KNN_NONE;
        }
    }
}

// The statistic of a row of k values and what the row is: a point's (its first value is not NaN), complete
// (its last value is not the padding).  The padding is +inf, so both statistics of an incomplete row come out +inf by their
// own arithmetic; the result says so outright.
__device__ __forceinline__ float knn_statistic(const float *__restrict__ row, uint32_t k, uint32_t kind, bool &point, bool &complete) {
    const float first = row[0], last = row[k - 1u];
    point = first == first;
    complete = point && f2u(last) != KNN_INF;
    if (!point) return first;
    if (!complete) return __builtin_inff();
    if (kind == KNN_KTH_DIST2) return last;
    float sum = sqrtf(first);
    for (uint32_t t = 1u; t < k; t++) sum = sum + sqrtf(row[t]);
    return sum / (float)k;
}

// sel = sel op {i : row i is a point's and lo <= v_i <= hi}: one thread per row, a wave's 64 results are two whole words of
// the mask (k_select_shape, k_nb_select)
__global__ __launch_bounds__(256) void k_knn_select(const float *__restrict__ plane, uint32_t n, uint32_t k, uint32_t kind, float lo,
                                                    float hi, uint32_t *__restrict__ words, uint32_t op) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool hit = false;
    if (i < n) {
        bool point, complete;
        const float v = knn_statistic(plane + (uint64_t)i * k, k, kind, point, complete);
        hit = point && lo <= v && v <= hi;
    }
    const uint64_t m = __ballot(hit);
    const uint32_t lane = threadIdx.x & 63u, word = i >> 5;
    if ((lane & 31u) == 0u && i < n) words[word] = sel_apply(words[word], (uint32_t)(m >> lane), op);
}

// ---- gs_knn_summary: the partial / finish shape of gs_gaussians_buffer_stats (gs_stats_kernels.h) ----------------------------

// part_u[f * nblocks + block], f = 0: points, 1: complete rows, 2: the smallest v's bits, 3: the largest v's bits + 1 (0: no
// complete row); part_d[f * nblocks + block], f = 0: the sum of v, 1: of v v.  v of a complete row is finite and >= +0, so the
// unsigned order of its bits is the bit order of the definition.
constexpr uint32_t KNN_U_FIELDS = 4u, KNN_D_FIELDS = 2u;

// what the finishing kernel leaves on the device: the layout of gs_knn_summary_result (include/gs3d.h)
struct KnnSummaryOut {
    uint64_t points, complete;
    uint32_t min_bits, max_bits;
    double sum, sum_sq;
};

// One thread per row.  Wave reductions, then the four waves through LDS in wave order.
__global__ __launch_bounds__(256) void k_knn_summary_partial(const float *__restrict__ plane, uint32_t n, uint32_t k, uint32_t kind,
                                                             uint32_t *__restrict__ part_u, double *__restrict__ part_d,
                                                             uint32_t nblocks) {
    __shared__ uint32_t s_u[4][KNN_U_FIELDS];
    __shared__ double s_d[4][KNN_D_FIELDS];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    bool point = false, complete = false;
    float v = 0.0f;
    if (i < n) v = knn_statistic(plane + (uint64_t)i * k, k, kind, point, complete);
    const double vd = complete ? (double)v : 0.0;
    const uint32_t pts = wave_reduce_add(point ? 1u : 0u), cpl = wave_reduce_add(complete ? 1u : 0u);
    const uint32_t mn = wave_reduce_min(complete ? f2u(v) : KNN_INF), mx = wave_reduce_max(complete ? f2u(v) + 1u : 0u);
    const double sm = wave_reduce_add_f64(vd), sq = wave_reduce_add_f64(vd * vd);
    if (lane == 0u) {
        s_u[wid][0] = pts;
        s_u[wid][1] = cpl;
        s_u[wid][2] = mn;
        s_u[wid][3] = mx;
        s_d[wid][0] = sm;
        s_d[wid][1] = sq;
    }
    __syncthreads();
    const uint32_t f = threadIdx.x;
    if (f < KNN_U_FIELDS) {
        const uint32_t x0 = s_u[0][f], x1 = s_u[1][f], x2 = s_u[2][f], x3 = s_u[3][f];
        part_u[(uint64_t)f * nblocks + blockIdx.x] = f < 2u ? (x0 + x1) + (x2 + x3) : f == 2u ? min(min(x0, x1), min(x2, x3)) : max(max(x0, x1), max(x2, x3));
    } else if (f >= 64u && f < 64u + KNN_D_FIELDS) {
        const uint32_t d = f - 64u;
        part_d[(uint64_t)d * nblocks + blockIdx.x] = (s_d[0][d] + s_d[1][d]) + (s_d[2][d] + s_d[3][d]);
    }
}

// One workgroup.  Thread t takes the partial rows t, t + 256, ... in ascending order; the 256 running values are reduced across
// the wave and then across the four waves in wave order.  The shape depends on nblocks alone, so the sums are the same bits
// from run to run.
__global__ __launch_bounds__(256) void k_knn_summary_finish(const uint32_t *__restrict__ part_u, const double *__restrict__ part_d,
                                                            uint32_t nblocks, KnnSummaryOut *__restrict__ out) {
    __shared__ uint64_t s_c[4][2];
    __shared__ uint32_t s_m[4][2];
    __shared__ double s_d[4][KNN_D_FIELDS];
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    uint64_t pts = 0ull, cpl = 0ull;
    uint32_t mn = KNN_INF, mx = 0u;
    double sm = 0.0, sq = 0.0;
    for (uint32_t b = threadIdx.x; b < nblocks; b += 256u) {
        pts += part_u[b];
        cpl += part_u[(uint64_t)nblocks + b];
        mn = min(mn, part_u[2ull * nblocks + b]);
        mx = max(mx, part_u[3ull * nblocks + b]);
        sm = sm + part_d[b];
        sq = sq + part_d[(uint64_t)nblocks + b];
    }
    pts = wave_reduce_add64(pts);
    cpl = wave_reduce_add64(cpl);
    mn = wave_reduce_min(mn);
    mx = wave_reduce_max(mx);
    sm = wave_reduce_add_f64(sm);
    sq = wave_reduce_add_f64(sq);
    if (lane == 0u) {
        s_c[wid][0] = pts;
        s_c[wid][1] = cpl;
        s_m[wid][0] = mn;
        s_m[wid][1] = mx;
        s_d[wid][0] = sm;
        s_d[wid][1] = sq;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        out->points = (s_c[0][0] + s_c[1][0]) + (s_c[2][0] + s_c[3][0]);
        out->complete = (s_c[0][1] + s_c[1][1]) + (s_c[2][1] + s_c[3][1]);
        const uint32_t m1 = max(max(s_m[0][1], s_m[1][1]), max(s_m[2][1], s_m[3][1]));
        out->min_bits = min(min(s_m[0][0], s_m[1][0]), min(s_m[2][0], s_m[3][0]));
        out->max_bits = m1 ? m1 - 1u : 0xff800000u;      // -inf: no complete row
        out->sum = (s_d[0][0] + s_d[1][0]) + (s_d[2][0] + s_d[3][0]);
        out->sum_sq = (s_d[0][1] + s_d[1][1]) + (s_d[2][1] + s_d[3][1]);
    }
}

}  // namespace gs
