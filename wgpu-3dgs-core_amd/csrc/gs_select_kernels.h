// gs_select_kernels.h — Gaussian selections (include/gs3d.h gs_selection): a bit per Gaussian in CALLER
// index order (bit i & 31 of word i >> 5), the select ops that fill it, and the gather into the renderer's mirror-slot
// order that the preprocess kernels read (SelIO, gs_render_kernels.h).  No reference item: the reference's viewer and
// editor keep such a buffer; the core crate does not.
#pragma once

#include "gs_render_kernels.h"

namespace gs {

enum { SEL_SET = 0, SEL_OR = 1, SEL_AND = 2, SEL_ANDNOT = 3, SEL_XOR = 4 };

// dst op src on one word.  A source word never has bits at positions >= n, so neither has the result.
__device__ __forceinline__ uint32_t sel_apply(uint32_t d, uint32_t s, uint32_t op) {
    return op == SEL_SET ? s : op == SEL_OR ? d | s : op == SEL_AND ? d & s : op == SEL_ANDNOT ? d & ~s : d ^ s;
}

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

// sphere: P = {center xyz, radius^2}; box: P = world_to_box, column-major 3 x 4
struct SelectShape {
    float M[16];   // model_transform_mat
    float P[12];
};

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

// gs_renderer_select_visible: the per-slot outputs a frame left behind -> bits of a scratch plane in caller index order
struct VisibleIO {
    const uint32_t *depth;         // per-slot depth keys (0xffffffff = culled)
    const uint32_t *chunk_vis;     // 0 = the chunk's per-slot arrays are stale (block-culled or fully hidden)
    const uint32_t *recs;          // blend records: words 0, 1 = mx, my
    const uint32_t *block_list;    // list frame: block of every list position; else null
    const uint32_t *list_blocks;   // ... and the list's length (device word)
    const uint32_t *order;         // caller index of every mirror slot; null = identity
    uint32_t n, nslots;
    float x0, y0, x1, y1;
    const uint8_t *mask;           // H x W, or null
    uint32_t width, height;
    uint32_t *scratch;             // cleared; bits are set with atomics (the slots of one word are scattered)
};

__global__ __launch_bounds__(256) void k_select_visible(VisibleIO io) {
    const uint32_t slot = blockIdx.x * 256u + threadIdx.x;
    const uint32_t limit = io.block_list ? *io.list_blocks * (uint32_t)PP_CHUNK : io.nslots;
    if (slot >= limit || slot >= io.nslots) return;
    if (io.chunk_vis[slot / (uint32_t)PP_CHUNK] == 0u || io.depth[slot] == 0xffffffffu) return;
    const float mx = u2f(io.recs[(uint64_t)slot * REC_WORDS]), my = u2f(io.recs[(uint64_t)slot * REC_WORDS + 1u]);
    if (!(io.x0 <= mx && mx < io.x1 && io.y0 <= my && my < io.y1)) return;
    if (io.mask) {
        if (!(mx >= 0.0f && my >= 0.0f && mx < (float)io.width && my < (float)io.height)) return;
        const uint32_t px = (uint32_t)floorf(mx), py = (uint32_t)floorf(my);
        if (px >= io.width || py >= io.height || io.mask[(uint64_t)py * io.width + px] == 0u) return;
    }
    uint32_t ms = slot;
    if (io.block_list) ms = io.block_list[slot / (uint32_t)PP_CHUNK] * (uint32_t)PP_CHUNK + slot % (uint32_t)PP_CHUNK;
    if (ms >= io.n) return;
    const uint32_t i = io.order ? io.order[ms] : ms;
    if (i >= io.n) return;
    atomicOr(&io.scratch[i >> 5], 1u << (i & 31u));
}

// Caller-order mask -> mirror-slot order, 64 slots per word (SelIO), one workgroup per 1024-block of the mirror; with
// `block_hidden`, also the block's "every Gaussian is hidden" flag.  out holds blocks * 16 words.
__global__ __launch_bounds__(PP_THREADS) void k_selection_to_slots(const uint32_t *__restrict__ words,
                                                                   const uint32_t *__restrict__ order, uint32_t n,
                                                                   uint64_t *__restrict__ out,
                                                                   uint32_t *__restrict__ block_hidden) {
    __shared__ uint32_t s_all[PP_THREADS / WAVE];
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    bool all = true;
#pragma unroll
    for (int k = 0; k < PP_ITEMS; k++) {
        const uint32_t slot = blockIdx.x * (uint32_t)PP_CHUNK + k * PP_THREADS + threadIdx.x;
        bool bit = false;
        if (slot < n) {
            const uint32_t i = order ? order[slot] : slot;
            bit = i < n && ((words[i >> 5] >> (i & 31u)) & 1u);
        }
        const uint64_t m = __ballot(bit), valid = __ballot(slot < n);
        if (lane == 0u) out[slot >> 6] = m;
        all = all && m == valid;
    }
    if (!block_hidden) return;
    if (lane == 0u) s_all[wid] = all ? 1u : 0u;
    __syncthreads();
    if (threadIdx.x == 0u) block_hidden[blockIdx.x] = (s_all[0] & s_all[1]) & (s_all[2] & s_all[3]);
}

}  // namespace gs
