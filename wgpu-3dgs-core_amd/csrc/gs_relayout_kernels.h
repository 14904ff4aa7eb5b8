// gs_relayout_kernels.h — layout conversion fused with the stable compaction of an extraction (include/gs3d.h
// gs_gaussians_buffer_create_converted / _create_concat_as).  No reference item: a buffer of the reference
// keeps the layout it was uploaded with.
//
// The per-record arithmetic is convert_words (gs_pack_kernels.h), shared with the host path gs_convert_pods: the device
// result is bit-equal to the host's by construction.  The same holds for k_decompose_extract (gs_gaussians_buffer_create_decomposed,
// DESIGN.md §3.12a) and decompose_words / gs_decompose_pods.
#pragma once

#include "gs_pack_kernels.h"

namespace gs {

// words between two records of the kernel's LDS image: room for the larger of the two layouts, and = 4 (mod 8), so that the
// 16-byte accesses of 16 neighbouring records (one lane group of a ds_read_b128 / ds_write_b128) fall on 64 different banks
__host__ __device__ constexpr int relayout_stride(int ssh, int dsh) {
    const int a = pod_words(ssh, COV_ROT_SCALE), b = pod_words(dsh, COV_ROT_SCALE), m = a > b ? a : b;
    return m % 8 == 0 ? m + 4 : m;
}

// One workgroup per 256 source Gaussians, one wave per 64, located as in k_extract_copy: lanes 0..31 hold the 32 mask words of
// the wave's 1024-block, their popcount prefix plus offsets[block] (k_scan_chunks) is the rank of the wave's first selected
// Gaussian.  The records of the wave's selected Gaussians — the others are not loaded — enter LDS through coalesced 16-byte
// loads, all in flight at once, packed by rank; lane r converts record r from LDS to registers to the same LDS slot (convert_words, SH configs
// constant, cov configs uniform); the converted records, contiguous in the destination, leave as one span of 16-byte
// stores at dst_base + rank.  Destination order = caller order (stable).  `total` bounds the ranks: a selection that another
// stream changed behind the count (the caller's error) loses records instead of writing past the end.
// snc / dnc: 16-byte chunks per source / destination record.
template <int SSH, int DSH>
__global__ __launch_bounds__(256) void k_convert_extract(const uint4 *__restrict__ src, uint4 *__restrict__ dst,
                                                         const uint32_t *__restrict__ words, uint32_t n, uint32_t invert,
                                                         const uint32_t *__restrict__ offsets, int scov, int dcov,
                                                         uint64_t dst_base, uint32_t total) {
    constexpr int STRIDE = relayout_stride(SSH, DSH);                 // words
    constexpr int SNC_MAX = pod_words(SSH, COV_ROT_SCALE) / 4, DNC_MAX = pod_words(DSH, COV_ROT_SCALE) / 4;
    __shared__ uint4 s_rec[256 * STRIDE / 4];                          // <= 60 KiB
    const uint32_t lane = threadIdx.x & 63u, wave0 = threadIdx.x - lane;
    const uint32_t i0 = blockIdx.x * 256u + wave0;                     // first Gaussian of the wave
    const uint32_t snc = (uint32_t)pod_words(SSH, scov) / 4u, dnc = (uint32_t)pod_words(DSH, dcov) / 4u;
    uint64_t mask = 0ull, base = 0ull;
    if (i0 < n) {
        const uint32_t block = i0 / PLANAR_BLOCK, wsel = (i0 % PLANAR_BLOCK) >> 5;
        const uint32_t word = lane < 32u ? extract_word(words, block * 32u + lane, n, invert) : 0u;
        const uint32_t pc = (uint32_t)__popc(word);
        const uint32_t inc = wave_inclusive_scan(pc, lane);
        const uint32_t lo = (uint32_t)__shfl((int)word, (int)wsel), hi = (uint32_t)__shfl((int)word, (int)wsel + 1);
        const uint32_t before = (uint32_t)__shfl((int)(inc - pc), (int)wsel);
        mask = (uint64_t)lo | ((uint64_t)hi << 32);
        base = (uint64_t)offsets[block] + before;
    }
    const uint32_t cnt = (uint32_t)__popcll(mask);                     // the wave's selected Gaussians (wave-uniform)
    uint4 *slot0 = s_rec + wave0 * (STRIDE / 4);                       // the wave's 64 slots
    if (cnt) {
        // the wave's span is snc x 64 chunks: lane takes chunk lane + 64 j.  All loads are issued before the first LDS store
        // (two loops, both unrolled): at two workgroups per CU a load-then-store loop would pay one HBM latency per step.
        const uint4 *s = src + (uint64_t)i0 * snc;
        uint32_t v[SNC_MAX][4], at[SNC_MAX];       // at: where chunk j goes in the wave's slots; ~0: not selected
#pragma unroll
        for (int j = 0; j < SNC_MAX; j++) {
            const uint32_t q = lane + 64u * (uint32_t)j;
            const uint32_t r = (q / snc) & 63u, c = q - (q / snc) * snc;
            const bool take = (uint32_t)j < snc && ((mask >> r) & 1ull);
            at[j] = take ? (uint32_t)__popcll(mask & ((1ull << r) - 1ull)) * (STRIDE / 4) + c : 0xffffffffu;
            uint4 x = make_uint4(0u, 0u, 0u, 0u);
            if (take) x = s[q];
            v[j][0] = x.x;
            v[j][1] = x.y;
            v[j][2] = x.z;
            v[j][3] = x.w;
        }
#pragma unroll
        for (int j = 0; j < SNC_MAX; j++)
            if (at[j] != 0xffffffffu) slot0[at[j]] = make_uint4(v[j][0], v[j][1], v[j][2], v[j][3]);
    }
    __syncthreads();
    if (lane < cnt) {
        uint4 *rec = slot0 + lane * (STRIDE / 4);
        uint32_t w[SNC_MAX * 4], o[DNC_MAX * 4];
#pragma unroll
        for (int c = 0; c < SNC_MAX; c++) {
            const uint4 v = (uint32_t)c < snc ? rec[c] : make_uint4(0u, 0u, 0u, 0u);
            w[4 * c] = v.x;
            w[4 * c + 1] = v.y;
            w[4 * c + 2] = v.z;
            w[4 * c + 3] = v.w;
        }
        convert_words(SSH, scov, DSH, dcov, w, o);
#pragma unroll
        for (int c = 0; c < DNC_MAX; c++)
            if ((uint32_t)c < dnc) rec[c] = make_uint4(o[4 * c], o[4 * c + 1], o[4 * c + 2], o[4 * c + 3]);
    }
    __syncthreads();
    if (cnt) {
        uint4 *d = dst + (dst_base + base) * dnc;
        for (uint32_t q = lane; q < cnt * dnc; q += 64u) {
            const uint32_t r = q / dnc, c = q - r * dnc;
            if (base + r < total) d[q] = slot0[r * (STRIDE / 4) + c];
        }
    }
}

// The frame of k_convert_extract with decompose_words per record: (SSH, scov), scov f32 or f16, ->
// (DSH, rot-scale).  The frame is written out again, not shared: k_convert_extract keeps its device code instruction for
// instruction (a shared frame taking the per-record function as a parameter was tried; hipcc then scheduled all 16 of its
// instances differently).  Location, loads, LDS image, store span and the `total` bound are those described above.
// New per lane: cov3d_decompose — six matrix terms and the nine of V in registers, the pair order written out (nothing is
// indexed at run time), a fixed number of sweeps (uniform across the wave), skipped rotations as selects.  Its 18 rotations
// cost 54 correctly rounded divisions and 36 square roots per record.
template <int SSH, int DSH>
__global__ __launch_bounds__(256) void k_decompose_extract(const uint4 *__restrict__ src, uint4 *__restrict__ dst,
                                                           const uint32_t *__restrict__ words, uint32_t n, uint32_t invert,
                                                           const uint32_t *__restrict__ offsets, int scov, uint64_t dst_base,
                                                           uint32_t total) {
    constexpr int STRIDE = relayout_stride(SSH, DSH);                 // words
    constexpr int SNC_MAX = pod_words(SSH, COV_ROT_SCALE) / 4, DNC = pod_words(DSH, COV_ROT_SCALE) / 4;
    __shared__ uint4 s_rec[256 * STRIDE / 4];                          // <= 60 KiB
    const uint32_t lane = threadIdx.x & 63u, wave0 = threadIdx.x - lane;
    const uint32_t i0 = blockIdx.x * 256u + wave0;                     // first Gaussian of the wave
    const uint32_t snc = (uint32_t)pod_words(SSH, scov) / 4u;
    uint64_t mask = 0ull, base = 0ull;
    if (i0 < n) {
        const uint32_t block = i0 / PLANAR_BLOCK, wsel = (i0 % PLANAR_BLOCK) >> 5;
        const uint32_t word = lane < 32u ? extract_word(words, block * 32u + lane, n, invert) : 0u;
        const uint32_t pc = (uint32_t)__popc(word);
        const uint32_t inc = wave_inclusive_scan(pc, lane);
        const uint32_t lo = (uint32_t)__shfl((int)word, (int)wsel), hi = (uint32_t)__shfl((int)word, (int)wsel + 1);
        const uint32_t before = (uint32_t)__shfl((int)(inc - pc), (int)wsel);
        mask = (uint64_t)lo | ((uint64_t)hi << 32);
        base = (uint64_t)offsets[block] + before;
    }
    const uint32_t cnt = (uint32_t)__popcll(mask);                     // the wave's selected Gaussians (wave-uniform)
    uint4 *slot0 = s_rec + wave0 * (STRIDE / 4);                       // the wave's 64 slots
    if (cnt) {
        const uint4 *s = src + (uint64_t)i0 * snc;
        uint32_t v[SNC_MAX][4], at[SNC_MAX];       // at: where chunk j goes in the wave's slots; ~0: not selected
#pragma unroll
        for (int j = 0; j < SNC_MAX; j++) {
            const uint32_t q = lane + 64u * (uint32_t)j;
            const uint32_t r = (q / snc) & 63u, c = q - (q / snc) * snc;
            const bool take = (uint32_t)j < snc && ((mask >> r) & 1ull);
            at[j] = take ? (uint32_t)__popcll(mask & ((1ull << r) - 1ull)) * (STRIDE / 4) + c : 0xffffffffu;
            uint4 x = make_uint4(0u, 0u, 0u, 0u);
            if (take) x = s[q];
            v[j][0] = x.x;
            v[j][1] = x.y;
            v[j][2] = x.z;
            v[j][3] = x.w;
        }
#pragma unroll
        for (int j = 0; j < SNC_MAX; j++)
            if (at[j] != 0xffffffffu) slot0[at[j]] = make_uint4(v[j][0], v[j][1], v[j][2], v[j][3]);
    }
    __syncthreads();
    if (lane < cnt) {
        uint4 *rec = slot0 + lane * (STRIDE / 4);
        uint32_t w[SNC_MAX * 4], o[DNC * 4];
#pragma unroll
        for (int c = 0; c < SNC_MAX; c++) {
            const uint4 v = (uint32_t)c < snc ? rec[c] : make_uint4(0u, 0u, 0u, 0u);
            w[4 * c] = v.x;
            w[4 * c + 1] = v.y;
            w[4 * c + 2] = v.z;
            w[4 * c + 3] = v.w;
        }
        decompose_words(SSH, scov, DSH, w, o, DeviceSqrt());
#pragma unroll
        for (int c = 0; c < DNC; c++) rec[c] = make_uint4(o[4 * c], o[4 * c + 1], o[4 * c + 2], o[4 * c + 3]);
    }
    __syncthreads();
    if (cnt) {
        uint4 *d = dst + (dst_base + base) * DNC;
        for (uint32_t q = lane; q < cnt * DNC; q += 64u) {
            const uint32_t r = q / DNC, c = q - r * DNC;
            if (base + r < total) d[q] = slot0[r * (STRIDE / 4) + c];
        }
    }
}

}  // namespace gs
