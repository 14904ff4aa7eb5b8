// gs_neighbor_kernels.h — neighbour counts of the device editor (include/gs3d.h gs_gaussians_buffer_neighbor_counts,
// gs_select_neighbors): for every POINT (a Gaussian of `among` whose transformed position is finite) the
// number of other points within a radius, decided by the binary32 test (dx dx + dy dy) + dz dz <= fl(r r).  No reference
// item: the reference's editor removes floaters on the host from its own copy of the Gaussians.
//
// The count is defined without a grid; the grid only bounds the candidates.  Every point gets a cell of 21 bits per axis
// over the bounding box of the points, of side h >= r (1 + 2^-10); the key (qz << 42) | (qy << 21) | qx is sorted with
// the device radix sort, so a ROW of cells (fixed qy, qz) is one contiguous run of the sorted order and the 27 cells
// around a query are 9 such runs.  DESIGN.md §3.11 shows that two neighbours differ by at most one cell per axis.
// Every operation is rounded (-ffp-contract=off).
#pragma once

#include "gs_neighbor_grid.h"

namespace gs {

// pw of Gaussian i and whether it is a point; `among` = its bit of the mask
__device__ __forceinline__ bool nb_point(const uint32_t *__restrict__ aos, uint32_t pod_words, uint32_t i, const float M[16],
                                         bool among, float pw[4]) {
    const uint32_t *w = aos + (uint64_t)i * pod_words;
    const float p[3] = {u2f(w[0]), u2f(w[1]), u2f(w[2])};
    mat4_mul_point(M, p, pw);
    return among && attr_finite(pw[0]) && attr_finite(pw[1]) && attr_finite(pw[2]);
}

// k_bbox_partial over the transformed positions of the points; partial[block][6] = lo xyz, hi xyz (+inf / -inf: no point)
__global__ __launch_bounds__(256) void k_nb_bbox_partial(const uint32_t *__restrict__ aos, uint32_t pod_words, uint32_t n,
                                                         const uint32_t *__restrict__ among, SelectShape sh,
                                                         float *__restrict__ partial) {
    __shared__ float s_lo[4][3], s_hi[4][3];
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    for (uint64_t base = (uint64_t)blockIdx.x * 256u; base < n; base += (uint64_t)gridDim.x * 256u) {
        const uint32_t i = (uint32_t)base + threadIdx.x;
        const uint64_t mask = wave_selection_mask(among, i - lane, n);
        float pw[4];
        if (i < n && nb_point(aos, pod_words, i, sh.M, (mask >> lane) & 1ull, pw)) {
#pragma unroll
            for (int a = 0; a < 3; a++) {
                lo[a] = fminf(lo[a], pw[a]);
                hi[a] = fmaxf(hi[a], pw[a]);
            }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
#pragma unroll
        for (int d = WAVE / 2; d > 0; d >>= 1) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], d, WAVE));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], d, WAVE));
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            s_lo[wid][a] = lo[a];
            s_hi[wid][a] = hi[a];
        }
    }
    __syncthreads();
    if (threadIdx.x < 3u) {
        const uint32_t a = threadIdx.x;
        partial[blockIdx.x * 6u + a] = fminf(fminf(s_lo[0][a], s_lo[1][a]), fminf(s_lo[2][a], s_lo[3][a]));
        partial[blockIdx.x * 6u + 3u + a] = fmaxf(fmaxf(s_hi[0][a], s_hi[1][a]), fmaxf(s_hi[2][a], s_hi[3][a]));
    }
}

// (nb_grid and nb_cell, the cell side and the cell of a coordinate: gs_neighbor_grid.h)

// keys[i] = the cell key of Gaussian i (NB_KEY_NONE: not a point), vals[i] = i
__global__ __launch_bounds__(256) void k_nb_keys(const uint32_t *__restrict__ aos, uint32_t pod_words, uint32_t n,
                                                 const uint32_t *__restrict__ among, SelectShape sh,
                                                 const float *__restrict__ bbox, float radius, uint64_t *__restrict__ keys,
                                                 uint32_t *__restrict__ vals) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    const uint64_t mask = wave_selection_mask(among, i - lane, n);
    if (i >= n) return;
    float pw[4];
    uint64_t key = NB_KEY_NONE;
    if (nb_point(aos, pod_words, i, sh.M, (mask >> lane) & 1ull, pw)) {
        double lo[3];
        const double inv_h = nb_grid(bbox, radius, lo);
        key = ((uint64_t)nb_cell(pw[2], lo[2], inv_h) << (2u * NB_CELL_BITS)) | ((uint64_t)nb_cell(pw[1], lo[1], inv_h) << NB_CELL_BITS) |
              (uint64_t)nb_cell(pw[0], lo[0], inv_h);
    }
    keys[i] = key;
    vals[i] = i;
}

// the transformed positions in sorted order, one plane per axis (NaN where the slot holds no point)
__global__ __launch_bounds__(256) void k_nb_gather(const uint32_t *__restrict__ aos, uint32_t pod_words, uint32_t n, SelectShape sh,
                                                   const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                   float *__restrict__ sx, float *__restrict__ sy, float *__restrict__ sz) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= n) return;
    float pw[4] = {__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), 0.0f};
    if (keys[s] != NB_KEY_NONE) (void)nb_point(aos, pod_words, vals[s], sh.M, true, pw);
    sx[s] = pw[0];
    sy[s] = pw[1];
    sz[s] = pw[2];
}

// counts[vals[s]] = min(c, cap) for the point in sorted slot s; MARK: NB_NOT_A_POINT instead of 0 where there is no point.
//
// A wave holds 64 consecutive sorted queries in registers.  It takes them in GROUPS: the first query not yet done and those
// behind it in the same row of cells, at most NB_SPAN cells further in x (consecutive lanes, the order is sorted).  For a
// group the 9 rows around it each hold ONE run of candidates — cells x_first - 1 .. x_last + 1 — whose two ends lanes 0..17
// find by binary search side by side.  The run is loaded 64 candidates at a time, one per lane and contiguous, and every
// lane of the group tests all of them (v_readlane: the candidate is wave-uniform).  A candidate that passes the test IS a
// neighbour whatever its cell, and the runs of a group are disjoint, so nothing is counted twice; the query itself is
// skipped by its slot.  A group stops once all its queries have reached `cap`.
template <bool MARK>
__global__ __launch_bounds__(256) void k_nb_count(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                  const float *__restrict__ sx, const float *__restrict__ sy,
                                                  const float *__restrict__ sz, uint32_t n, float rr, uint32_t cap,
                                                  uint32_t *__restrict__ counts) {
    const uint32_t lane = threadIdx.x & 63u, s = blockIdx.x * 256u + threadIdx.x;
    const uint64_t key = s < n ? keys[s] : NB_KEY_NONE;
    const bool point = key != NB_KEY_NONE;
    const uint32_t qx = (uint32_t)key & NB_CELL_MAX, row_lo = (uint32_t)(key >> NB_CELL_BITS), row_hi = (uint32_t)(key >> (NB_CELL_BITS + 32u));
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    if (point) {
        px = sx[s];
        py = sy[s];
        pz = sz[s];
    }
    uint32_t cnt = 0u;
    uint64_t todo = __ballot(point);
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
        bool more = true;
        for (uint32_t k = 0u; k < 9u && more; k++) {
            const uint32_t begin = nb_readlane(lo, 2u * k), end = nb_readlane(lo, 2u * k + 1u);
            for (uint32_t t = begin; t < end && more; t += 64u) {
                const uint32_t c = t + lane, m = end - t < 64u ? end - t : 64u;
                float cx = 0.0f, cy = 0.0f, cz = 0.0f;
                if (c < end) {
                    cx = sx[c];
                    cy = sy[c];
                    cz = sz[c];
                }
                for (uint32_t j = 0u; j < m; j++) {
                    const float dx = px - nb_readlane_f(cx, j), dy = py - nb_readlane_f(cy, j), dz = pz - nb_readlane_f(cz, j);
                    const bool hit = (dx * dx + dy * dy) + dz * dz <= rr;
                    if (in && hit && t + j != s && cnt < cap) cnt++;
                }
                more = __any(in && cnt < cap);
            }
        }
    }
    if (s < n) counts[vals[s]] = point ? cnt : (MARK ? NB_NOT_A_POINT : 0u);
}

// sel = sel op {i : counts[i] is a point's and lo <= counts[i] <= hi}, caller order: a wave's 64 results are two whole
// words of the mask (k_select_shape)
__global__ __launch_bounds__(256) void k_nb_select(const uint32_t *__restrict__ counts, uint32_t n, uint32_t lo, uint32_t hi,
                                                   uint32_t *__restrict__ words, uint32_t op) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool hit = false;
    if (i < n) {
        const uint32_t c = counts[i];
        hit = c != NB_NOT_A_POINT && lo <= c && c <= hi;
    }
    const uint64_t m = __ballot(hit);
    const uint32_t lane = threadIdx.x & 63u, word = i >> 5;
    if ((lane & 31u) == 0u && i < n) words[word] = sel_apply(words[word], (uint32_t)(m >> lane), op);
}

}  // namespace gs
