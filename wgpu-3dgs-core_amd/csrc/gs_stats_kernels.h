// gs_stats_kernels.h — the read side of the device editor (include/gs3d.h gs_gaussians_buffer_stats / _histogram,
// gs_select_attribute): reductions over one binary32 ATTRIBUTE of the selected records of the caller-order
// AoS buffer.  No reference item: the reference's editor computes bounds, centroids and histograms on the host from its
// own copy of the Gaussians; the core crate has none.
//
// The records are decoded with gs_kernel_lib.h (mat4_mul_point, unorm8, gaussian_unpack_cov3d); the mask is read and
// written word-wise as in gs_select_kernels.h / gs_edit_kernels.h.  Every operation is rounded (-ffp-contract=off).
#pragma once

#include "gs_device_common.h"

namespace gs {

enum : uint32_t {
    ATTR_X = 0, ATTR_Y = 1, ATTR_Z = 2, ATTR_RED = 3, ATTR_GREEN = 4, ATTR_BLUE = 5, ATTR_OPACITY = 6, ATTR_SIZE2 = 7,
    ATTR_DIST2 = 8, ATTR_COUNT = 9
};
// what a pass over ONE attribute reads of a record: words 0..2, word 3, or the layout's covariance words
enum : int { ATTR_CLASS_POS = 0, ATTR_CLASS_COLOR = 1, ATTR_CLASS_COV = 2 };

__host__ __device__ constexpr int attr_class(uint32_t attr) {
    return attr == ATTR_SIZE2 ? ATTR_CLASS_COV : (attr >= ATTR_RED && attr <= ATTR_OPACITY) ? ATTR_CLASS_COLOR : ATTR_CLASS_POS;
}

struct AttrArgs {
    float M[16];      // model_transform_mat
    float ref[3];     // DIST2
    uint32_t attr;
};

// the total order on the bit patterns as an unsigned integer: -0 < +0, every finite key lies strictly between the keys
// of -inf and +inf
__device__ __forceinline__ uint32_t attr_sort_key(float v) {
    const uint32_t u = f2u(v);
    return (u & 0x80000000u) ? ~u : u | 0x80000000u;
}
__host__ __device__ __forceinline__ uint32_t attr_key_bits(uint32_t key) { return (key & 0x80000000u) ? key ^ 0x80000000u : ~key; }
constexpr uint32_t ATTR_KEY_POS_INF = 0xff800000u, ATTR_KEY_NEG_INF = 0x007fffffu;     // identities of min / max

__device__ __forceinline__ float attr_size2(const float c6[6]) { return (c6[0] + c6[3]) + c6[5]; }
__device__ __forceinline__ float attr_dist2(const float pw[4], const float ref[3]) {
    const float dx = pw[0] - ref[0], dy = pw[1] - ref[1], dz = pw[2] - ref[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// the attribute of one record; only the words of its class are loaded
template <int CLS, int SH, int COV>
__device__ __forceinline__ float attr_value(const uint32_t *__restrict__ rec, const AttrArgs &a) {
    if constexpr (CLS == ATTR_CLASS_POS) {
        const float p[3] = {u2f(rec[0]), u2f(rec[1]), u2f(rec[2])};
        float pw[4];
        mat4_mul_point(a.M, p, pw);
        return a.attr == ATTR_X ? pw[0] : a.attr == ATTR_Y ? pw[1] : a.attr == ATTR_Z ? pw[2] : attr_dist2(pw, a.ref);
    } else if constexpr (CLS == ATTR_CLASS_COLOR) {
        return (float)((rec[3] >> (8u * (a.attr - ATTR_RED))) & 0xffu) / 255.0f;      // unorm8
    } else {
        float c6[6];
        gaussian_unpack_cov3d<SH, COV>(rec, c6);
        return attr_size2(c6);
    }
}

// wave_selection_mask made uniform for the compiler too: the branches on it are scalar branches
__device__ __forceinline__ uint64_t wave_selection_mask_uniform(const uint32_t *__restrict__ words, uint32_t i0, uint32_t n) {
    const uint64_t m = wave_selection_mask(words, i0, n);
    return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)m) |
           ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(m >> 32)) << 32);
}

// (wave_reduce_add_f64, the wave sum of a double in a fixed shape: gs_device_common.h, shared with gs_knn_kernels.h)

// ---- gs_select_attribute -------------------------------------------------------------------------------------------

// sel = sel op {i : lo <= v_i && v_i <= hi}: one thread per Gaussian, the wave's 64 results are two whole words of the
// mask (k_select_shape).  AND and ANDNOT keep no Gaussian that is not selected already, so such a wave reads its two
// words first, returns when they are 0 and evaluates only the Gaussians whose bit is set.  NaN compares false.
template <int CLS, int SH, int COV>
__global__ __launch_bounds__(256) void k_select_attr(const uint32_t *__restrict__ aos, uint32_t pod_words, uint32_t n, AttrArgs a,
                                                     float lo, float hi, uint32_t *__restrict__ words, uint32_t op) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    uint64_t need = ~0ull;
    if (op == SEL_AND || op == SEL_ANDNOT) {
        need = wave_selection_mask_uniform(words, i - lane, n);
        if (need == 0ull) return;
    }
    bool hit = false;
    if (i < n && ((need >> lane) & 1ull)) {
        const float v = attr_value<CLS, SH, COV>(aos + (uint64_t)i * pod_words, a);
        hit = lo <= v && v <= hi;
    }
    const uint64_t m = __ballot(hit);
    const uint32_t word = i >> 5;
    if ((lane & 31u) == 0u && i < n) words[word] = sel_apply(words[word], (uint32_t)(m >> lane), op);
}

// ---- gs_gaussians_buffer_histogram ---------------------------------------------------------------------------------

// NaN -> bins + 2, v < lo -> bins, v >= hi -> bins + 1, else trunc((v - lo) scale) clamped to bins - 1
__device__ __forceinline__ uint32_t attr_hist_slot(float v, float lo, float hi, float scale, uint32_t bins) {
    if (v != v) return bins + 2u;
    if (v < lo) return bins;
    if (v >= hi) return bins + 1u;
    const uint32_t b = (uint32_t)((v - lo) * scale);
    return b < bins - 1u ? b : bins - 1u;
}

// Two rows of bins + 3 counters in LDS (dynamic: 8 (bins + 3) bytes), row 0 = the selected Gaussians, row 1 = the others;
// a workgroup strides over the buffer 256 Gaussians at a time and adds its non-zero counters to the global u64 rows once,
// with integer atomics (the result does not depend on their order).  A workgroup sees fewer than 2^32 Gaussians.
template <int CLS, int SH, int COV>
__global__ __launch_bounds__(256) void k_histogram(const uint32_t *__restrict__ aos, uint32_t pod_words, uint32_t n,
                                                   const uint32_t *__restrict__ words, AttrArgs a, float lo, float hi, float scale,
                                                   uint32_t bins, unsigned long long *__restrict__ out) {
    extern __shared__ uint32_t s_hist[];
    const uint32_t row = bins + 3u, lane = threadIdx.x & 63u;
    for (uint32_t k = threadIdx.x; k < 2u * row; k += 256u) s_hist[k] = 0u;
    __syncthreads();
    for (uint64_t base = (uint64_t)blockIdx.x * 256u; base < n; base += (uint64_t)gridDim.x * 256u) {
        const uint32_t i = (uint32_t)base + threadIdx.x;
        const uint64_t mask = wave_selection_mask(words, i - lane, n);
        if (i < n) {
            const float v = attr_value<CLS, SH, COV>(aos + (uint64_t)i * pod_words, a);
            const uint32_t slot = attr_hist_slot(v, lo, hi, scale, bins);
            atomicAdd(&s_hist[((mask >> lane) & 1ull) ? slot : row + slot], 1u);
        }
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < 2u * row; k += 256u) {
        const uint32_t c = s_hist[k];
        if (c) atomicAdd(&out[k], (unsigned long long)c);
    }
}

// ---- gs_gaussians_buffer_stats -------------------------------------------------------------------------------------

// One partial row per workgroup, field-major: part_u[f * nblocks + block], f = 0: count, 1 + k: finite values of
// attribute k, 10 + k: its smallest sort key, 19 + k: its largest; part_d[k * nblocks + block]: its sum.
constexpr uint32_t STATS_U_FIELDS = 1u + 3u * ATTR_COUNT;

// One thread per Gaussian; a selected record is decoded once for all nine attributes.  Wave reductions, then the four
// waves through LDS in wave order.  A wave without a selected Gaussian reads its two mask words and no record.
template <int SH, int COV>
__global__ __launch_bounds__(256) void k_stats_partial(const uint32_t *__restrict__ aos, uint32_t n, const uint32_t *__restrict__ words,
                                                       AttrArgs a, uint32_t *__restrict__ part_u, double *__restrict__ part_d,
                                                       uint32_t nblocks) {
    __shared__ uint32_t s_u[4][STATS_U_FIELDS];
    __shared__ double s_d[4][ATTR_COUNT];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    const uint64_t mask = wave_selection_mask_uniform(words, i - lane, n);
    uint32_t fin[ATTR_COUNT], mn[ATTR_COUNT], mx[ATTR_COUNT];
    double sm[ATTR_COUNT];
#pragma unroll
    for (int k = 0; k < (int)ATTR_COUNT; k++) {
        fin[k] = 0u;
        mn[k] = ATTR_KEY_POS_INF;
        mx[k] = ATTR_KEY_NEG_INF;
        sm[k] = 0.0;
    }
    if (mask != 0ull) {
        if ((mask >> lane) & 1ull) {      // (bits at positions >= n are never set)
            const uint32_t *rec = aos + (uint64_t)i * (uint32_t)pod_words(SH, COV);
            const uint4 head = *(const uint4 *)rec;
            const float p[3] = {u2f(head.x), u2f(head.y), u2f(head.z)};
            float pw[4], c6[6];
            mat4_mul_point(a.M, p, pw);
            gaussian_unpack_cov3d<SH, COV>(rec, c6);
            const float v[ATTR_COUNT] = {pw[0], pw[1], pw[2], unorm8(head.w, 0), unorm8(head.w, 1), unorm8(head.w, 2),
                                         unorm8(head.w, 3), attr_size2(c6), attr_dist2(pw, a.ref)};
#pragma unroll
            for (int k = 0; k < (int)ATTR_COUNT; k++) {
                if (attr_finite(v[k])) {
                    fin[k] = 1u;
                    mn[k] = mx[k] = attr_sort_key(v[k]);
                    sm[k] = (double)v[k];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < (int)ATTR_COUNT; k++) {
            fin[k] = wave_reduce_add(fin[k]);
            mn[k] = wave_reduce_min(mn[k]);
            mx[k] = wave_reduce_max(mx[k]);
            sm[k] = wave_reduce_add_f64(sm[k]);
        }
    }
    if (lane == 0u) {
        s_u[wid][0] = (uint32_t)__popcll(mask);
#pragma unroll
        for (int k = 0; k < (int)ATTR_COUNT; k++) {
            s_u[wid][1 + k] = fin[k];
            s_u[wid][1 + ATTR_COUNT + k] = mn[k];
            s_u[wid][1 + 2 * ATTR_COUNT + k] = mx[k];
            s_d[wid][k] = sm[k];
        }
    }
    __syncthreads();
    const uint32_t f = threadIdx.x;
    if (f < STATS_U_FIELDS) {
        const uint32_t x0 = s_u[0][f], x1 = s_u[1][f], x2 = s_u[2][f], x3 = s_u[3][f];
        uint32_t r;
        if (f < 1u + ATTR_COUNT) r = (x0 + x1) + (x2 + x3);
        else if (f < 1u + 2u * ATTR_COUNT) r = min(min(x0, x1), min(x2, x3));
        else r = max(max(x0, x1), max(x2, x3));
        part_u[(uint64_t)f * nblocks + blockIdx.x] = r;
    } else if (f >= 64u && f < 64u + ATTR_COUNT) {
        const uint32_t k = f - 64u;
        part_d[(uint64_t)k * nblocks + blockIdx.x] = (s_d[0][k] + s_d[1][k]) + (s_d[2][k] + s_d[3][k]);
    }
}

// what the finishing kernel leaves on the device: the layout of gs_stats (include/gs3d.h)
struct StatsOut {
    uint64_t count;
    struct {
        uint64_t finite;
        uint32_t min_bits, max_bits;
        double sum;
    } attr[ATTR_COUNT];
};

// One workgroup.  Thread t takes the partial rows t, t + 256, ... in ascending order; the 256 running values are
// reduced across the wave and then across the four waves in wave order.  The shape depends on nblocks alone, so the
// sums are the same bits from run to run.
__global__ __launch_bounds__(256) void k_stats_finish(const uint32_t *__restrict__ part_u, const double *__restrict__ part_d,
                                                      uint32_t nblocks, StatsOut *__restrict__ out) {
    __shared__ uint64_t s_c[4][1 + ATTR_COUNT];
    __shared__ uint32_t s_m[4][2 * ATTR_COUNT];
    __shared__ double s_d[4][ATTR_COUNT];
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    uint64_t cnt[1 + ATTR_COUNT];
    uint32_t mn[ATTR_COUNT], mx[ATTR_COUNT];
    double sm[ATTR_COUNT];
#pragma unroll
    for (int k = 0; k < (int)ATTR_COUNT; k++) {
        mn[k] = ATTR_KEY_POS_INF;
        mx[k] = ATTR_KEY_NEG_INF;
        sm[k] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < 1 + (int)ATTR_COUNT; k++) cnt[k] = 0ull;
    for (uint32_t b = threadIdx.x; b < nblocks; b += 256u) {
#pragma unroll
        for (int k = 0; k < 1 + (int)ATTR_COUNT; k++) cnt[k] += part_u[(uint64_t)k * nblocks + b];
#pragma unroll
        for (int k = 0; k < (int)ATTR_COUNT; k++) {
            mn[k] = min(mn[k], part_u[(uint64_t)(1 + ATTR_COUNT + k) * nblocks + b]);
            mx[k] = max(mx[k], part_u[(uint64_t)(1 + 2 * ATTR_COUNT + k) * nblocks + b]);
            sm[k] = sm[k] + part_d[(uint64_t)k * nblocks + b];
        }
    }
#pragma unroll
    for (int k = 0; k < 1 + (int)ATTR_COUNT; k++) cnt[k] = wave_reduce_add64(cnt[k]);
#pragma unroll
    for (int k = 0; k < (int)ATTR_COUNT; k++) {
        mn[k] = wave_reduce_min(mn[k]);
        mx[k] = wave_reduce_max(mx[k]);
        sm[k] = wave_reduce_add_f64(sm[k]);
    }
    if (lane == 0u) {
#pragma unroll
        for (int k = 0; k < 1 + (int)ATTR_COUNT; k++) s_c[wid][k] = cnt[k];
#pragma unroll
        for (int k = 0; k < (int)ATTR_COUNT; k++) {
            s_m[wid][k] = mn[k];
            s_m[wid][ATTR_COUNT + k] = mx[k];
            s_d[wid][k] = sm[k];
        }
    }
    __syncthreads();
    const uint32_t k = threadIdx.x;
    if (k == 0u) out->count = (s_c[0][0] + s_c[1][0]) + (s_c[2][0] + s_c[3][0]);
    if (k < ATTR_COUNT) {
        out->attr[k].finite = (s_c[0][1 + k] + s_c[1][1 + k]) + (s_c[2][1 + k] + s_c[3][1 + k]);
        out->attr[k].min_bits = attr_key_bits(min(min(s_m[0][k], s_m[1][k]), min(s_m[2][k], s_m[3][k])));
        out->attr[k].max_bits = attr_key_bits(max(max(s_m[0][ATTR_COUNT + k], s_m[1][ATTR_COUNT + k]),
                                                  max(s_m[2][ATTR_COUNT + k], s_m[3][ATTR_COUNT + k])));
        out->attr[k].sum = (s_d[0][k] + s_d[1][k]) + (s_d[2][k] + s_d[3][k]);
    }
}

}  // namespace gs
