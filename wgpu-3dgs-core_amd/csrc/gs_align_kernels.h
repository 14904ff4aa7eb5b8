// gs_align_kernels.h — nearest neighbours between two buffers and the correspondence sums of a rigid fit (include/gs3d.h
// gs_gaussians_buffer_knn_between, gs_gaussians_buffer_pair_sums): for every QUERY of one buffer the k
// smallest binary32 squared distances to the points of ANOTHER buffer within a radius, with the target caller indices they
// belong to, ordered by (bits of d2, target caller index).  No reference item: the reference has no neighbour search.
//
// The row is defined without a grid.  The target's sorted cell grid (gs_neighbor_grid.h, the front of gs_neighbors.hip)
// bounds the candidates; a query gets its cell IN THAT GRID, from the target's bounding box and cell side, and the query
// keys are sorted the same way, so 64 consecutive sorted queries lie in few rows of cells and search together.
// Every operation is rounded (-ffp-contract=off).
#pragma once

#include "gs_neighbor_grid.h"

namespace gs {

// (the constants of a row are those of gs_knn_kernels.h, which belongs to another unit: one kernel header, one unit)
constexpr uint32_t AL_MAX_K = 16u;
constexpr uint32_t AL_NONE = 0xffffffffu;        // GS_KNN_NONE
constexpr uint32_t AL_INF = 0x7f800000u;         // +inf: the distance of a padding entry
constexpr uint32_t AL_NAN = 0x7fc00000u;         // every distance of a written row that belongs to no point
constexpr uint64_t AL_PAD = ((uint64_t)AL_INF << 32) | AL_NONE;
// the three query keys that are no cell; a cell key has 63 bits, so all of them sort behind every cell
constexpr uint64_t AL_KEY_SKIP = ~0ull;          // not in `queries`: nothing is written
constexpr uint64_t AL_KEY_NO_POINT = ~0ull - 1u; // a query whose pw is not finite: a row of NaN / NONE
constexpr uint64_t AL_KEY_FAR = ~0ull - 2u;      // a query point that can have no candidate: a row of +inf / NONE

// pw of Gaussian i of a buffer and whether it is finite (nb_point of gs_neighbor_kernels.h, the same arithmetic)
__device__ __forceinline__ bool al_point(const uint32_t *__restrict__ aos, uint32_t pod_words, uint32_t i, const float M[16], float pw[4]) {
    const uint32_t *w = aos + (uint64_t)i * pod_words;
    const float p[3] = {u2f(w[0]), u2f(w[1]), u2f(w[2])};
    mat4_mul_point(M, p, pw);
    return attr_finite(pw[0]) && attr_finite(pw[1]) && attr_finite(pw[2]);
}

// The cell of a query coordinate in the target's grid, or -1: no target point can be its neighbour.
//   u = fl64(fl64(v - lo) fl64(1 / h)) is the arithmetic of nb_cell; c = floor(u), c_hi = floor(u(hi)) = the largest cell of a
//   target point (u is monotone in v).  DESIGN.md §3.11 shows |u_a - u_b| < 1 for two neighbours while |u| <= 2^22, so their
//   floors differ by at most 1 (§3.19 extends it to u < 0).  Hence: c < -1 or c > c_hi + 1 has no candidate (FAR; |u| > 2^22
//   is far by more than 2^21 cells); c = -1 is keyed as cell 0, whose three cells -1..1 hold cell 0, the only one a candidate
//   can be in; c >= 2^21 - 1 is keyed as the last cell, as nb_cell clamps the targets, and a candidate's cell >= c - 1 is then
//   the last cell or the one before it.
__device__ __forceinline__ int32_t al_query_cell(float v, double lo, double hi, double inv_h) {
    const double c = floor(((double)v - lo) * inv_h), c_hi = floor((hi - lo) * inv_h);
    if (!(c >= -1.0) || c > c_hi + 1.0) return -1;
    return c >= (double)NB_CELL_MAX ? (int32_t)NB_CELL_MAX : (c > 0.0 ? (int32_t)c : 0);
}

// keys[i] = the key of query i: its cell in the target's grid, or one of AL_KEY_*; vals[i] = i.  tbbox: the bounding box of
// the target's points (k_bbox_final: lo > hi on every axis when it has none); null: the target has no Gaussian at all.
__global__ __launch_bounds__(256) void k_al_query_keys(const uint32_t *__restrict__ aos, uint32_t pod_words, uint32_t n,
                                                       const uint32_t *__restrict__ queries, SelectShape sh,
                                                       const float *__restrict__ tbbox, float radius, uint64_t *__restrict__ keys,
                                                       uint32_t *__restrict__ vals) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    const uint64_t mask = wave_selection_mask(queries, i - lane, n);
    if (i >= n) return;
    uint64_t key = AL_KEY_SKIP;
    if ((mask >> lane) & 1ull) {
        float pw[4];
        key = AL_KEY_NO_POINT;
        if (al_point(aos, pod_words, i, sh.M, pw)) {
            key = AL_KEY_FAR;
            if (tbbox && tbbox[0] <= tbbox[3] && tbbox[1] <= tbbox[4] && tbbox[2] <= tbbox[5]) {
                double lo[3];
                const double inv_h = nb_grid(tbbox, radius, lo);
                const int32_t cx = al_query_cell(pw[0], lo[0], (double)tbbox[3], inv_h), cy = al_query_cell(pw[1], lo[1], (double)tbbox[4], inv_h),
                              cz = al_query_cell(pw[2], lo[2], (double)tbbox[5], inv_h);
                if (cx >= 0 && cy >= 0 && cz >= 0)
                    key = ((uint64_t)(uint32_t)cz << (2u * NB_CELL_BITS)) | ((uint64_t)(uint32_t)cy << NB_CELL_BITS) | (uint64_t)(uint32_t)cx;
            }
        }
    }
    keys[i] = key;
    vals[i] = i;
}

// the transformed positions of the queries in sorted order, one plane per axis (NaN where the slot searches nothing)
__global__ __launch_bounds__(256) void k_al_query_gather(const uint32_t *__restrict__ aos, uint32_t pod_words, uint32_t n, SelectShape sh,
                                                         const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                         float *__restrict__ sx, float *__restrict__ sy, float *__restrict__ sz) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= n) return;
    float pw[4] = {__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), 0.0f};
    if (keys[s] < AL_KEY_FAR) (void)al_point(aos, pod_words, vals[s], sh.M, pw);
    sx[s] = pw[0];
    sy[s] = pw[1];
    sz[s] = pw[2];
}

// The traversal of k_nb_knn<K> (gs_knn_kernels.h) with two changes: the queries (qkeys, qvals, qx, qy, qz: nq sorted slots)
// are arrays of their own beside the candidates (tkeys, tvals, tx, ty, tz: nt sorted slots of the target's grid), and no
// candidate is excluded by its slot.  The rest is kept: 64 sorted queries per wave, groups of one row of cells at most NB_SPAN
// cells long, 18 binary searches side by side over the TARGET keys, the 9 runs streamed 64 candidates at a time and
// broadcast by v_readlane, a lane's K best entries ascending in e[0..K) as 64-bit words (bits of d2 << 32) | target caller
// index, the compare-exchange chain, skipped for the whole wave when no lane accepts.  Every load is guarded (s < nq,
// c < end <= nt, mid < nt).  dist2[i K + t], index[i K + t]: row i in QUERY caller order; index may be null.
template <int K>
__global__ __launch_bounds__(256) void k_nb_knn_between(const uint64_t *__restrict__ tkeys, const uint32_t *__restrict__ tvals,
                                                        const float *__restrict__ tx, const float *__restrict__ ty,
                                                        const float *__restrict__ tz, uint32_t nt,
                                                        const uint64_t *__restrict__ qkeys, const uint32_t *__restrict__ qvals,
                                                        const float *__restrict__ qxs, const float *__restrict__ qys,
                                                        const float *__restrict__ qzs, uint32_t nq, float rr,
                                                        uint32_t *__restrict__ dist2, uint32_t *__restrict__ index) {
    const uint32_t lane = threadIdx.x & 63u, s = blockIdx.x * 256u + threadIdx.x;
    uint64_t key = AL_KEY_SKIP;
    uint32_t self = 0u;
    if (s < nq) {
        key = qkeys[s];
        self = qvals[s];
    }
    const bool query = key != AL_KEY_SKIP;
    if (!__any(query)) return;
    const bool point = key != AL_KEY_SKIP && key != AL_KEY_NO_POINT, searches = key < AL_KEY_FAR;
    const uint32_t qx = (uint32_t)key & NB_CELL_MAX, row_lo = (uint32_t)(key >> NB_CELL_BITS), row_hi = (uint32_t)(key >> (NB_CELL_BITS + 32u));
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    if (searches) {
        px = qxs[s];
        py = qys[s];
        pz = qzs[s];
    }
    uint64_t e[K];
#pragma unroll
    for (int t = 0; t < K; t++) e[t] = AL_PAD;
    uint64_t todo = __ballot(searches);
    while (todo) {
        const uint32_t leader = (uint32_t)__builtin_ctzll(todo);
        const uint32_t l_lo = nb_readlane(row_lo, leader), l_hi = nb_readlane(row_hi, leader), l_qx = nb_readlane(qx, leader);
        const bool in = ((todo >> lane) & 1ull) && row_lo == l_lo && row_hi == l_hi && qx - l_qx <= NB_SPAN;
        const uint64_t group = __ballot(in);      // (the leader's bit at least)
        todo &= ~group;
        const uint32_t last_qx = nb_readlane(qx, 63u - (uint32_t)__builtin_clzll(group));
        const uint32_t x0 = l_qx ? l_qx - 1u : 0u, x1 = last_qx < NB_CELL_MAX ? last_qx + 1u : NB_CELL_MAX;
        const uint32_t l_qy = l_lo & NB_CELL_MAX, l_qz = (uint32_t)((((uint64_t)l_hi << 32) | l_lo) >> NB_CELL_BITS);
        // lane 2 k: the first target slot of row k with cell x >= x0; lane 2 k + 1: the first slot behind its cells x <= x1
        const uint32_t k9 = lane >> 1;
        const int32_t cz = (int32_t)l_qz + (int32_t)(k9 / 3u) - 1, cy = (int32_t)l_qy + (int32_t)(k9 % 3u) - 1;
        const bool search = lane < 18u && cz >= 0 && cz <= (int32_t)NB_CELL_MAX && cy >= 0 && cy <= (int32_t)NB_CELL_MAX;
        const bool upper = lane & 1u;
        const uint64_t target = ((uint64_t)(uint32_t)cz << (2u * NB_CELL_BITS)) | ((uint64_t)(uint32_t)cy << NB_CELL_BITS) | (upper ? x1 : x0);
        uint32_t lo = 0u, hi = search ? nt : 0u;      // (a row outside the grid: the empty run [0, 0))
        while (__any(lo < hi)) {
            if (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2u;
                const uint64_t k = tkeys[mid];
                if (upper ? k <= target : k < target) lo = mid + 1u;
                else hi = mid;
            }
        }
        for (uint32_t k = 0u; k < 9u; k++) {
            const uint32_t begin = nb_readlane(lo, 2u * k), end = nb_readlane(lo, 2u * k + 1u);
            for (uint32_t t = begin; t < end; t += 64u) {
                const uint32_t c = t + lane, m = end - t < 64u ? end - t : 64u;
                float cx = 0.0f, cyv = 0.0f, czv = 0.0f;
                uint32_t cv = 0u;
                if (c < end) {
                    cx = tx[c];
                    cyv = ty[c];
                    czv = tz[c];
                    cv = tvals[c];
                }
                for (uint32_t j = 0u; j < m; j++) {
                    const float dx = px - nb_readlane_f(cx, j), dy = py - nb_readlane_f(cyv, j), dz = pz - nb_readlane_f(czv, j);
                    const float d2 = (dx * dx + dy * dy) + dz * dz;
                    // (the exact test against e[K - 1], index included, is the chain's own first comparison)
                    const bool maybe = in && d2 <= rr && f2u(d2) <= (uint32_t)(e[K - 1] >> 32);
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
    if (query) {      // (s < nq)
        const uint64_t row = (uint64_t)self * (uint32_t)K;
#pragma unroll
        for (int t = 0; t < K; t++) {
            dist2[row + t] = point ? (uint32_t)(e[t] >> 32) : AL_NAN;
            if (index) index[row + t] = point ? (uint32_t)e[t] : AL_NONE;
        }
    }
}

// ---- gs_gaussians_buffer_pair_sums: the partial / finish shape of gs_gaussians_buffer_stats (gs_stats_kernels.h) ------------

// the sums of a pair (p, q) in the order of gs_pair_sums behind its count: sp[3], sq[3], spq[9] row-major, spp, sqq, sdd
constexpr uint32_t AL_D_FIELDS = 18u;

// what the finishing kernel leaves on the device: the layout of gs_pair_sums (include/gs3d.h)
struct PairSumsOut {
    uint64_t pairs;
    double d[AL_D_FIELDS];
};

struct PairShapes {
    float Mq[16], Mt[16];      // model_transform_mat of the query side and of the target side
};

// One thread per query i.  j = index_plane[i k] is dereferenced only when j < nt; both pw in binary32, then widened; every
// product is exact in binary64, the squares of a vector are added (x x + y y) + z z.  Wave reductions, then the four waves
// through LDS in wave order.  part_u[block] = pairs, part_d[f * nblocks + block].
__global__ __launch_bounds__(256) void k_al_pair_partial(const uint32_t *__restrict__ qaos, uint32_t q_words, uint32_t nq,
                                                         const uint32_t *__restrict__ queries, const uint32_t *__restrict__ taos,
                                                         uint32_t t_words, uint32_t nt, PairShapes sh,
                                                         const uint32_t *__restrict__ index_plane, uint32_t k,
                                                         uint32_t *__restrict__ part_u, double *__restrict__ part_d, uint32_t nblocks) {
    __shared__ uint32_t s_u[4];
    __shared__ double s_d[4][AL_D_FIELDS];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    const uint64_t mask = wave_selection_mask(queries, i - lane, nq);
    double v[AL_D_FIELDS];
#pragma unroll
    for (int f = 0; f < (int)AL_D_FIELDS; f++) v[f] = 0.0;
    bool pair = false;
    if (i < nq && ((mask >> lane) & 1ull)) {
        const uint32_t j = index_plane[(uint64_t)i * k];
        float pf[4], qf[4];
        if (j < nt && al_point(qaos, q_words, i, sh.Mq, pf) && al_point(taos, t_words, j, sh.Mt, qf)) {
            pair = true;
            const double p[3] = {(double)pf[0], (double)pf[1], (double)pf[2]}, q[3] = {(double)qf[0], (double)qf[1], (double)qf[2]};
            const double d[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
#pragma unroll
            for (int a = 0; a < 3; a++) {
                v[a] = p[a];
                v[3 + a] = q[a];
#pragma unroll
                for (int b = 0; b < 3; b++) v[6 + 3 * a + b] = p[a] * q[b];
            }
            v[15] = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2];
            v[16] = (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2];
            v[17] = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
        }
    }
    const uint32_t cnt = wave_reduce_add(pair ? 1u : 0u);
#pragma unroll
    for (int f = 0; f < (int)AL_D_FIELDS; f++) v[f] = wave_reduce_add_f64(v[f]);
    if (lane == 0u) {
        s_u[wid] = cnt;
#pragma unroll
        for (int f = 0; f < (int)AL_D_FIELDS; f++) s_d[wid][f] = v[f];
    }
    __syncthreads();
    const uint32_t f = threadIdx.x;
    if (f < AL_D_FIELDS) part_d[(uint64_t)f * nblocks + blockIdx.x] = (s_d[0][f] + s_d[1][f]) + (s_d[2][f] + s_d[3][f]);
    else if (f == 64u) part_u[blockIdx.x] = (s_u[0] + s_u[1]) + (s_u[2] + s_u[3]);
}

// One workgroup.  Thread t takes the partial rows t, t + 256, ... in ascending order; the 256 running values are reduced across
// the wave and then across the four waves in wave order.  The shape depends on nblocks alone, so the sums are the same bits
// from run to run.
__global__ __launch_bounds__(256) void k_al_pair_finish(const uint32_t *__restrict__ part_u, const double *__restrict__ part_d,
                                                        uint32_t nblocks, PairSumsOut *__restrict__ out) {
    __shared__ uint64_t s_c[4];
    __shared__ double s_d[4][AL_D_FIELDS];
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    uint64_t cnt = 0ull;
    double v[AL_D_FIELDS];
#pragma unroll
    for (int f = 0; f < (int)AL_D_FIELDS; f++) v[f] = 0.0;
    for (uint32_t b = threadIdx.x; b < nblocks; b += 256u) {
        cnt += part_u[b];
#pragma unroll
        for (int f = 0; f < (int)AL_D_FIELDS; f++) v[f] = v[f] + part_d[(uint64_t)f * nblocks + b];
    }
    cnt = wave_reduce_add64(cnt);
#pragma unroll
    for (int f = 0; f < (int)AL_D_FIELDS; f++) v[f] = wave_reduce_add_f64(v[f]);
    if (lane == 0u) {
        s_c[wid] = cnt;
#pragma unroll
        for (int f = 0; f < (int)AL_D_FIELDS; f++) s_d[wid][f] = v[f];
    }
    __syncthreads();
    if (threadIdx.x == 0u) out->pairs = (s_c[0] + s_c[1]) + (s_c[2] + s_c[3]);
    if (threadIdx.x < AL_D_FIELDS) out->d[threadIdx.x] = (s_d[0][threadIdx.x] + s_d[1][threadIdx.x]) + (s_d[2][threadIdx.x] + s_d[3][threadIdx.x]);
}

}  // namespace gs
