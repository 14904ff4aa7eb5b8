// gs_component_kernels.h — connected components of the neighbour graph (include/gs3d.h gs_gaussians_buffer_components,
// gs_select_components, gs_select_connected): the points of §3.11 are the vertices, the neighbour pairs
// the edges; L_i = the smallest caller index of i's component, S_i = its number of points.  No reference item: the
// reference's editor has no cluster pass.
//
// The grid, the sort and the sorted positions are those of gs_neighbor_kernels.h (one front for both units); the link
// kernel walks the candidates exactly as k_nb_count does and unions the two ends of every passing pair in a lock-free
// union-find over SORTED SLOTS (neighbours lie near each other there).  The forest is safe under stale reads by
// construction, not by fences:
//   * inside the link launch a parent word is written only by agent-scope atomics (atomicCAS on a word that still names
//     itself, atomicMin) and read only by relaxed agent-scope atomic loads;
//   * a word only ever DECREASES, and only to a slot of the same component ("larger root under smaller"), so a stale
//     value is an older true link and "same root" concluded from stale reads is sound;
//   * a failed atomic continues from the value it returned, never from a reload: every retry moves strictly down in
//     index and every loop is finite (the loops also stop at a word that does not decrease, whatever it holds);
//   * no wave waits for another: no spin, no flag, no barrier across workgroups.  Kernel boundaries are the only
//     synchronisation, and plain loads of the words come only behind the boundary that follows the last write.
// Labels, sizes and the info are integer min / add / max / or: they depend on neither the traversal nor the run.
#pragma once

#include "gs_neighbor_grid.h"

namespace gs {

constexpr uint32_t CC_NONE = 0xffffffffu;      // GS_COMPONENT_NONE: the label of a Gaussian that is no point

__device__ __forceinline__ uint32_t cc_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root above x as the atomic loads show it (link launch); every step goes down in index
__device__ __forceinline__ uint32_t cc_find(const uint32_t *parent, uint32_t x) {
    for (;;) {
        const uint32_t p = cc_load(parent + x);
        if (p >= x) return x;
        x = p;
    }
}

// unites the components of a and b, the larger root under the smaller; returns a slot that both now lie under (the root
// the call saw last).  a + b decreases with every turn that does not return.
__device__ __forceinline__ uint32_t cc_unite(uint32_t *parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return a;
        if (a < b) {
            const uint32_t t = a;
            a = b;
            b = t;
        }
        const uint32_t old = atomicCAS(parent + a, a, b);
        if (old >= a) return b;      // == a: linked
        a = old;                     // a had been linked meanwhile: go on from where it points
    }
}

// parent[s] = s, the per-root words cleared, the info zeroed (no point: 0, 0, 0, CC_NONE)
__global__ __launch_bounds__(256) void k_cc_init(uint32_t n, uint32_t *__restrict__ parent, uint32_t *__restrict__ rootmin,
                                                 uint32_t *__restrict__ rootsize, uint32_t *__restrict__ info) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s < n) {
        parent[s] = s;
        rootmin[s] = CC_NONE;
        rootsize[s] = 0u;
    }
    if (info && s < 4u) info[s] = s == 3u ? CC_NONE : 0u;
}

// The traversal of k_nb_count (groups of queries of one row, 9 runs found by 18 binary searches side by side, candidates
// streamed 64 at a time and broadcast with v_readlane), with no cap and no early exit.  Every passing pair whose candidate
// sits in a LOWER sorted slot is united — each edge once.  A lane keeps the last root it saw above its query (`cur`: an
// older true ancestor is as good a start as the query), and the parent words of the 64 candidates are loaded with them:
// where a candidate's word already shows `cur`, both ends lie in one component and no atomic is issued.
__global__ __launch_bounds__(256) void k_cc_link(const uint64_t *__restrict__ keys, const float *__restrict__ sx,
                                                 const float *__restrict__ sy, const float *__restrict__ sz, uint32_t n, float rr,
                                                 uint32_t *parent) {
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
    uint32_t cur = s;
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
        // the first query of the group sits in the lowest slot: a run is only of interest below the last query's slot
        const uint32_t s_last = blockIdx.x * 256u + (threadIdx.x & ~63u) + 63u - (uint32_t)__builtin_clzll(group);
        for (uint32_t k = 0u; k < 9u; k++) {
            const uint32_t begin = nb_readlane(lo, 2u * k), end0 = nb_readlane(lo, 2u * k + 1u);
            const uint32_t end = end0 < s_last ? end0 : s_last;      // candidates in slots < s only
            for (uint32_t t = begin; t < end; t += 64u) {
                const uint32_t c = t + lane, m = end - t < 64u ? end - t : 64u;
                float cx = 0.0f, cy = 0.0f, cz = 0.0f;
                uint32_t cp = 0u;
                if (c < end) {
                    cx = sx[c];
                    cy = sy[c];
                    cz = sz[c];
                    cp = cc_load(parent + c);
                }
                for (uint32_t j = 0u; j < m; j++) {
                    const float dx = px - nb_readlane_f(cx, j), dy = py - nb_readlane_f(cy, j), dz = pz - nb_readlane_f(cz, j);
                    const bool hit = (dx * dx + dy * dy) + dz * dz <= rr;
                    const uint32_t pc = nb_readlane(cp, j);      // <= t + j, in the candidate's component
                    if (in && hit && t + j < s && pc != cur) {
                        const uint32_t r = cc_unite(parent, cur, pc);
                        // a candidate more than one step from the root: shorten its path (an ancestor, so the word decreases
                        // within the component)
                        if (pc != t + j && r < pc) (void)atomicMin(parent + (t + j), r);
                        cur = r;
                    }
                }
            }
        }
    }
    if (point && cur < s) (void)atomicMin(parent + s, cur);
}

// Behind the link launch (plain loads): root[s] = the root above the point in slot s; per root the smallest caller index
// and the number of points, or (SEEDS) whether a point of the component carries a seed bit.  The lanes of a wave that
// share a root issue one atomic together.
template <bool SEEDS>
__global__ __launch_bounds__(256) void k_cc_finalise(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                     const uint32_t *__restrict__ parent, uint32_t n, uint32_t *__restrict__ root,
                                                     uint32_t *rootmin, uint32_t *rootsize, const uint32_t *__restrict__ seeds) {
    const uint32_t lane = threadIdx.x & 63u, s = blockIdx.x * 256u + threadIdx.x;
    const bool point = s < n && keys[s] != NB_KEY_NONE;
    uint32_t r = CC_NONE, i = CC_NONE;
    bool seeded = false;
    if (point) {
        i = vals[s];
        r = s;
        for (;;) {
            const uint32_t p = parent[r];
            if (p >= r) break;
            r = p;
        }
        root[s] = r;
        if (SEEDS) seeded = (seeds[i >> 5] >> (i & 31u)) & 1u;
    }
    uint64_t todo = __ballot(point);
    while (todo) {
        const uint32_t leader = (uint32_t)__builtin_ctzll(todo);
        const uint32_t lr = nb_readlane(r, leader);
        const bool same = point && r == lr;
        const uint64_t grp = __ballot(same);
        todo &= ~grp;
        if (SEEDS) {
            if (__ballot(same && seeded) && lane == leader) (void)atomicOr(rootsize + lr, 1u);
        } else {
            uint32_t lowest = same ? i : CC_NONE;
#pragma unroll
            for (int d = WAVE / 2; d > 0; d >>= 1) {
                const uint32_t o = (uint32_t)__shfl_xor((int)lowest, d, WAVE);
                lowest = o < lowest ? o : lowest;
            }
            if (lane == leader) {
                (void)atomicMin(rootmin + lr, lowest);
                (void)atomicAdd(rootsize + lr, (uint32_t)__builtin_popcountll(grp));
            }
        }
    }
}

// caller order: labels[i] = rootmin[root] (CC_NONE: no point), sizes[i] = rootsize[root] (0: no point); the info's points,
// components and largest by one atomic each per wave.  Any of the three may be null.
__global__ __launch_bounds__(256) void k_cc_scatter(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals,
                                                    const uint32_t *__restrict__ root, const uint32_t *__restrict__ rootmin,
                                                    const uint32_t *__restrict__ rootsize, uint32_t n, uint32_t *__restrict__ labels,
                                                    uint32_t *__restrict__ sizes, uint32_t *info) {
    const uint32_t lane = threadIdx.x & 63u, s = blockIdx.x * 256u + threadIdx.x;
    const bool point = s < n && keys[s] != NB_KEY_NONE;
    uint32_t label = CC_NONE, size = 0u;
    bool is_root = false;
    if (point) {
        const uint32_t r = root[s];
        is_root = r == s;
        size = rootsize[r];
        if (labels) label = rootmin[r];
    }
    if (s < n) {
        const uint32_t i = vals[s];
        if (labels) labels[i] = label;
        if (sizes) sizes[i] = size;
    }
    if (info) {
        const uint64_t pts = __ballot(point), roots = __ballot(is_root);
        uint32_t largest = is_root ? size : 0u;
#pragma unroll
        for (int d = WAVE / 2; d > 0; d >>= 1) {
            const uint32_t o = (uint32_t)__shfl_xor((int)largest, d, WAVE);
            largest = o > largest ? o : largest;
        }
        if (lane == 0u && pts) {
            (void)atomicAdd(info + 0, (uint32_t)__builtin_popcountll(pts));
            if (roots) {
                (void)atomicAdd(info + 1, (uint32_t)__builtin_popcountll(roots));
                (void)atomicMax(info + 2, largest);
            }
        }
    }
}

// behind k_cc_scatter: info[3] = the smallest label among the components of the largest size
__global__ __launch_bounds__(256) void k_cc_largest_label(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ root,
                                                          const uint32_t *__restrict__ rootmin, const uint32_t *__restrict__ rootsize,
                                                          uint32_t n, uint32_t *info) {
    const uint32_t lane = threadIdx.x & 63u, s = blockIdx.x * 256u + threadIdx.x;
    uint32_t label = CC_NONE;
    if (s < n && keys[s] != NB_KEY_NONE && root[s] == s && rootsize[s] == info[2]) label = rootmin[s];
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)label, d, WAVE);
        label = o < label ? o : label;
    }
    if (lane == 0u && label != CC_NONE) (void)atomicMin(info + 3, label);
}

// sel = sel op {i : value[i] != 0 and lo <= value[i] <= hi}, caller order (value: S_i, or the seed flag of i's component;
// 0 where i is no point): a wave's 64 results are two whole words of the mask (k_nb_select)
__global__ __launch_bounds__(256) void k_cc_select(const uint32_t *__restrict__ value, uint32_t n, uint32_t lo, uint32_t hi,
                                                   uint32_t *__restrict__ words, uint32_t op) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool hit = false;
    if (i < n) {
        const uint32_t v = value[i];
        hit = v != 0u && lo <= v && v <= hi;
    }
    const uint64_t m = __ballot(hit);
    const uint32_t lane = threadIdx.x & 63u, word = i >> 5;
    if ((lane & 31u) == 0u && i < n) words[word] = sel_apply(words[word], (uint32_t)(m >> lane), op);
}

}  // namespace gs
