// gs_device_common.h — what the kernel headers of the render, pack, select, edit, relayout, stats, neighbour and k-NN units share beyond
// gs_kernel_lib.h (gs_bundle_kernels.h needs only that one): WAVE and PLANAR_BLOCK, the wave / block primitives,
// attr_finite, the selection-mask helpers (SEL_*, sel_apply, SelectShape, wave_selection_mask) and the two scalar encoders
// that both the pack kernels and the edit kernel use.  It holds no kernel: every *_kernels.h is included by exactly one
// translation unit of the library — but gs_pack_kernels.h, whose per-record functions the relayout unit
// shares with gs_core.hip — this header by eight of them.
#pragma once

#include "gs_kernel_lib.h"

namespace gs {

constexpr int WAVE = 64;
// the mirror's block (gs_render_kernels.h, "block-planar"); also the block of the extraction scans (gs_edit_kernels.h)
constexpr uint32_t PLANAR_BLOCK = 1024;

// ---------------------------------------------------------------------------------------------
// wave / block primitives
// ---------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t lane_id() {
    return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
}

// number of set bits of `mask` strictly below this lane
__device__ __forceinline__ uint32_t mbcnt(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                     __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// Wave64 inclusive scans on the DPP cross-lane path (no LDS traffic, one VALU instruction per step):
// row_shr 1/2/4/8 scan each 16-lane row, row_bcast15 carries the row totals into the odd rows
// (row mask 0xa) and row_bcast31 carries the lower half's total into the upper half (row mask 0xc).
// Lanes without a source keep `identity`.  (A __shfl_up ladder costs a ds_bpermute round trip per
// step: ~6 dependent LDS operations per scan.)
#define GS_DPP_STEP(OP, CTRL, ROWMASK)                                                             \
    v = OP(v, (uint32_t)__builtin_amdgcn_update_dpp((int)identity, (int)v, CTRL, ROWMASK, 0xf, false))
__device__ __forceinline__ uint32_t dpp_op_add(uint32_t a, uint32_t b) { return a + b; }
__device__ __forceinline__ uint32_t dpp_op_max(uint32_t a, uint32_t b) { return a > b ? a : b; }

__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v, uint32_t lane) {
    (void)lane;
    const uint32_t identity = 0u;
    GS_DPP_STEP(dpp_op_add, 0x111, 0xf);   // row_shr:1
    GS_DPP_STEP(dpp_op_add, 0x112, 0xf);   // row_shr:2
    GS_DPP_STEP(dpp_op_add, 0x114, 0xf);   // row_shr:4
    GS_DPP_STEP(dpp_op_add, 0x118, 0xf);   // row_shr:8
    GS_DPP_STEP(dpp_op_add, 0x142, 0xa);   // row_bcast:15
    GS_DPP_STEP(dpp_op_add, 0x143, 0xc);   // row_bcast:31
    return v;
}

__device__ __forceinline__ uint32_t wave_inclusive_max(uint32_t v) {
    const uint32_t identity = 0u;
    GS_DPP_STEP(dpp_op_max, 0x111, 0xf);
    GS_DPP_STEP(dpp_op_max, 0x112, 0xf);
    GS_DPP_STEP(dpp_op_max, 0x114, 0xf);
    GS_DPP_STEP(dpp_op_max, 0x118, 0xf);
    GS_DPP_STEP(dpp_op_max, 0x142, 0xa);
    GS_DPP_STEP(dpp_op_max, 0x143, 0xc);
    return v;
}
#undef GS_DPP_STEP

__device__ __forceinline__ uint32_t dpp_op_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
// wave minimum / maximum, uniform in every lane (all 64 lanes must be active)
__device__ __forceinline__ uint32_t wave_reduce_min(uint32_t v) {
    const uint32_t identity = 0xffffffffu;
#define GS_DPP_MIN(CTRL, ROWMASK) \
    v = dpp_op_min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)identity, (int)v, CTRL, ROWMASK, 0xf, false))
    GS_DPP_MIN(0x111, 0xf); GS_DPP_MIN(0x112, 0xf); GS_DPP_MIN(0x114, 0xf); GS_DPP_MIN(0x118, 0xf);
    GS_DPP_MIN(0x142, 0xa); GS_DPP_MIN(0x143, 0xc);
#undef GS_DPP_MIN
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ uint32_t wave_reduce_max(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_max(v), 63);
}

// wave total, uniform in every lane (all 64 lanes must be active)
__device__ __forceinline__ uint32_t wave_reduce_add(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_scan(v, 0u), 63);
}

// Exclusive scan over a 256-thread block; `smem` holds >= 4 words; returns exclusive prefix and
// the block total.  Ends with the LDS reusable after the caller's next barrier.
__device__ __forceinline__ uint32_t block_exclusive_scan_256(uint32_t v, uint32_t *smem,
                                                             uint32_t &total) {
    uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    uint32_t inc = wave_inclusive_scan(v, lane);
    if (lane == 63u) smem[wid] = inc;
    __syncthreads();
    uint32_t w0 = smem[0], w1 = smem[1], w2 = smem[2], w3 = smem[3];
    uint32_t wave_off = wid == 0 ? 0u : wid == 1 ? w0 : wid == 2 ? w0 + w1 : w0 + w1 + w2;
    total = w0 + w1 + w2 + w3;
    __syncthreads();
    return wave_off + inc - v;
}

// wave sum of a 64-bit value, uniform in every lane (all 64 lanes active)
__device__ __forceinline__ uint64_t wave_reduce_add64(uint64_t v) {
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1) v += __shfl_xor((unsigned long long)v, d, WAVE);
    return v;
}

// wave sum of a double in a fixed shape (a butterfly: both partners of a step add the same two values), uniform in
// every lane; all 64 lanes active (gs_stats_kernels.h, gs_knn_kernels.h)
__device__ __forceinline__ double wave_reduce_add_f64(double v) {
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1) v = v + __shfl_xor(v, d, WAVE);
    return v;
}

// finite binary32 (no Inf, no NaN), from the bits
__device__ __forceinline__ bool attr_finite(float v) { return (f2u(v) & 0x7f800000u) != 0x7f800000u; }

// ---------------------------------------------------------------------------------------------
// selection masks (gs_select_kernels.h): a bit per Gaussian in caller index order
// ---------------------------------------------------------------------------------------------

enum { SEL_SET = 0, SEL_OR = 1, SEL_AND = 2, SEL_ANDNOT = 3, SEL_XOR = 4 };

// dst op src on one word.  A source word never has bits at positions >= n, so neither has the result.
__device__ __forceinline__ uint32_t sel_apply(uint32_t d, uint32_t s, uint32_t op) {
    return op == SEL_SET ? s : op == SEL_OR ? d | s : op == SEL_AND ? d & s : op == SEL_ANDNOT ? d & ~s : d ^ s;
}

// sphere: P = {center xyz, radius^2}; box: P = world_to_box, column-major 3 x 4
struct SelectShape {
    float M[16];   // model_transform_mat
    float P[12];
};

// the selection words of the 64 Gaussians starting at `i0` (a multiple of 64) as one 64-bit mask; words == null selects
// every Gaussian below n.  A mask word never has bits at positions >= n.
__device__ __forceinline__ uint64_t wave_selection_mask(const uint32_t *__restrict__ words, uint32_t i0, uint32_t n) {
    if (i0 >= n) return 0ull;
    if (!words) return n - i0 >= 64u ? ~0ull : (1ull << (n - i0)) - 1ull;
    const uint32_t w = i0 >> 5;
    const uint64_t lo = words[w], hi = i0 + 32u < n ? words[w + 1u] : 0u;
    return lo | (hi << 32);
}

// word `w` of the mask that an extraction copies (gs_edit_kernels.h, gs_relayout_kernels.h): the selection (null: all), inverted if asked, bits >= n cleared
__device__ __forceinline__ uint32_t extract_word(const uint32_t *__restrict__ words, uint32_t w, uint32_t n, uint32_t invert) {
    if (w * 32u >= n) return 0u;
    const uint32_t valid = n - w * 32u >= 32u ? 0xffffffffu : (1u << (n - w * 32u)) - 1u;
    const uint32_t v = words ? words[w] : 0xffffffffu;
    return (invert ? ~v : v) & valid;
}

// ---------------------------------------------------------------------------------------------
// scalar encoders of the POD layouts (gs_pack_kernels.h pack_words, gs_edit_kernels.h edit_encode_sh)
// ---------------------------------------------------------------------------------------------

// IEEE binary32 -> binary16, round to nearest even (half 2.7.1 f16::from_f32; gaussian_config.rs:59,227)
__host__ __device__ inline uint16_t f32_to_f16_rtne_bits(uint32_t fbits) {
    const uint32_t f32infty = 255u << 23, f16max = (127u + 16u) << 23;
    const uint32_t magic = ((127u - 15u) + (23u - 10u) + 1u) << 23;
    const uint32_t sign = fbits & 0x80000000u;
    uint32_t u = fbits ^ sign;
    uint16_t o;
    if (u >= f16max) {
        o = (u > f32infty) ? (uint16_t)(0x7e00u | ((u >> 13) & 0x1ffu)) : (uint16_t)0x7c00u;
    } else if (u < (113u << 23)) {
        // subnormal / zero result: one float add against the magic constant does the rounding
        union { uint32_t u; float f; } a, m;
        a.u = u;
        m.u = magic;
        a.f += m.f;
        o = (uint16_t)(a.u - magic);
    } else {
        const uint32_t odd = (u >> 13) & 1u;
        u += ((uint32_t)(15 - 127) << 23) + 0xfffu;
        u += odd;
        o = (uint16_t)(u >> 13);
    }
    return (uint16_t)(o | (sign >> 16));
}

// GaussianShNorm8Config: (v * 127).clamp(-127, 127) as i8 — truncation toward zero, NaN -> 0
__host__ __device__ inline uint32_t sh_norm8_byte(float v) {
    float x = v * 127.0f;
    if (x != x) x = 0.0f;
    if (x < -127.0f) x = -127.0f;
    if (x > 127.0f) x = 127.0f;
    return (uint32_t)(uint8_t)(int8_t)(int)x;
}
}  // namespace gs
