// gs_select_kernels.h — Gaussian selections (include/gs3d.h gs_selection): a bit per Gaussian in CALLER
// index order (bit i & 31 of word i >> 5) and the select ops that fill it.  The gather into the renderer's mirror-slot
// order that the preprocess kernels read (SelIO) and the select op over a frame's outputs are the render unit's
// (gs_render_kernels.h); SEL_*, sel_apply and SelectShape are shared with other kernel headers (gs_device_common.h).  No
// reference item: the reference's viewer and editor keep such a buffer; the core crate does not.
#pragma once

#include "gs_device_common.h"

namespace gs {

// mode 0: clear, 1: fill, 2: invert, 3: keep (only the tail is masked: behind an upload).  tail_mask = the valid bits of the
// last word.
__global__ __launch_bounds__(256) void k_sel_unary(uint32_t *__restrict__ words, uint32_t nwords, uint32_t tail_mask,
                                                   uint32_t mode) {
    for (uint32_t w = blockIdx.x * 256u + threadIdx.x; w < nwords; w += gridDim.x * 256u) {
        const uint32_t v = mode == 0u ? 0u : mode == 1u ? 0xffffffffu : mode == 2u ? ~words[w] : words[w];
        words[w] = w + 1u == nwords ? v & tail_mask : v;
    }
}

__global__ __launch_bounds__(256) void k_sel_combine(uint32_t *__restrict__ dst, const uint32_t *__restrict__ src,
                                                     uint32_t nwords, uint32_t op) {
    for (uint32_t w = blockIdx.x * 256u + threadIdx.x; w < nwords; w += gridDim.x * 256u)
        dst[w] = sel_apply(dst[w], src[w], op);
}

// dst = dst op {i : start <= i < end} over whole words; end <= n, so no bit at a position >= n is ever set
__global__ __launch_bounds__(256) void k_sel_range(uint32_t *__restrict__ words, uint32_t nwords, uint32_t start, uint32_t end,
                                                   uint32_t op) {
    for (uint32_t w = blockIdx.x * 256u + threadIdx.x; w < nwords; w += gridDim.x * 256u) {
        const uint64_t w0 = (uint64_t)w * 32u;
        const uint64_t a = start > w0 ? start - w0 : 0u, b = end > w0 ? end - w0 : 0u;      // the range inside the word: [a, min(b, 32))
        uint32_t bits = 0u;
        if (a < 32u && b > a) bits = (b >= 32u ? 0xffffffffu : (1u << b) - 1u) & ~((1u << a) - 1u);
        words[w] = sel_apply(words[w], bits, op);
    }
}

// popcount of the whole mask, added to *total (cleared by the host in stream order)
__global__ __launch_bounds__(256) void k_sel_count(const uint32_t *__restrict__ words, uint32_t nwords,
                                                   unsigned long long *__restrict__ total) {
    __shared__ uint32_t s_c[4];
    uint32_t c = 0;
    for (uint32_t w = blockIdx.x * 256u + threadIdx.x; w < nwords; w += gridDim.x * 256u) c += (uint32_t)__popc(words[w]);
    c = wave_reduce_add(c);
    if ((threadIdx.x & 63u) == 0u) s_c[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0u) atomicAdd(total, (unsigned long long)((s_c[0] + s_c[1]) + (s_c[2] + s_c[3])));
}

// One thread per Gaussian of the AoS buffer (position = the first 12 bytes of a record); a wave's 64 results are two
// whole words of the mask, so the op is applied without atomics.  Every comparison is false for NaN.
template <bool BOX>
__global__ __launch_bounds__(256) void k_select_shape(const uint32_t *__restrict__ aos, uint32_t pod_words, uint32_t n,
                                                      SelectShape sh, uint32_t *__restrict__ words, uint32_t op) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool hit = false;
    if (i < n) {
        const uint32_t *w = aos + (uint64_t)i * pod_words;
        const float p[3] = {u2f(w[0]), u2f(w[1]), u2f(w[2])};
        float pw[4];
        mat4_mul_point(sh.M, p, pw);
        if constexpr (BOX) {
            float q[3];
#pragma unroll
            for (int r = 0; r < 3; r++) q[r] = ((sh.P[r] * pw[0] + sh.P[3 + r] * pw[1]) + sh.P[6 + r] * pw[2]) + sh.P[9 + r];
            hit = fabsf(q[0]) <= 1.0f && fabsf(q[1]) <= 1.0f && fabsf(q[2]) <= 1.0f;
        } else {
            const float dx = pw[0] - sh.P[0], dy = pw[1] - sh.P[1], dz = pw[2] - sh.P[2];
            hit = (dx * dx + dy * dy) + dz * dz <= sh.P[3];
        }
    }
    const uint64_t m = __ballot(hit);
    const uint32_t lane = threadIdx.x & 63u, word = i >> 5;
    if ((lane & 31u) == 0u && i < n) words[word] = sel_apply(words[word], (uint32_t)(m >> lane), op);
}

// gs_select_contribution: one thread per 16-byte record {u64 sum, u32 hits, f32 wmax}, one 16-byte load;
// kind 0: (float)sum * 2^-24 (u64 -> f32 to nearest even, the scale exact), 1: (float)hits, 2: wmax.  The mask is written as
// by k_select_shape.
__global__ __launch_bounds__(256) void k_select_contrib(const uint4 *__restrict__ recs, uint32_t n, uint32_t kind, float lo, float hi,
                                                        uint32_t *__restrict__ words, uint32_t op) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool hit = false;
    if (i < n) {
        const uint4 r = recs[i];
        float v;
        if (kind == 0u) v = __ull2float_rn(((unsigned long long)r.y << 32) | r.x) * 0x1p-24f;
        else if (kind == 1u) v = __uint2float_rn(r.z);
        else v = u2f(r.w);
        hit = lo <= v && v <= hi;
    }
    const uint64_t m = __ballot(hit);
    const uint32_t lane = threadIdx.x & 63u, word = i >> 5;
    if ((lane & 31u) == 0u && i < n) words[word] = sel_apply(words[word], (uint32_t)(m >> lane), op);
}

}  // namespace gs
