// gs_export_kernels.h — the records of a buffer (or of a selection of it) as PLY vertices or SPZ columns, encoded on the device
// (include/gs3d.h gs_gaussians_buffer_export_ply / _export_spz_decompressed).  No reference item: the reference
// downloads the buffer and encodes on the host (Gaussian::to_ply / to_spz, gaussian.rs:95-125, 227-352).
//
// The per-record arithmetic is gs_convert.h's gaussian_to_ply_words / gaussian_to_spz_bytes behind gs_pack_kernels.h's
// unpack_words, the functions the host path (download_gaussians, gs_gaussian_to_ply, gs_spz_encode_decompressed) runs: the
// device result is byte-equal to the host's by construction.
#pragma once

#include "gs_pack_kernels.h"

namespace gs {

// Gaussians per workgroup: two waves.  The front end is k_convert_extract's (gs_relayout_kernels.h); with four waves the
// LDS image of the PLY kernel (256 x 68 words) would pass the 64 KiB a workgroup may declare.
constexpr uint32_t EXPORT_GROUP = 128;

// words between two records of the LDS image: a multiple of 4 (the records enter through 16-byte stores), = 4 (mod 8) so that
// the 16-byte accesses of 16 neighbouring records fall on 64 different banks (relayout_stride's rule), and room for `words`
__host__ __device__ constexpr int export_stride(int words) {
    const int m = (words + 3) / 4 * 4;
    return m % 8 == 0 ? m + 4 : m;
}

// The front end both kernels share.  The wave's 64 source Gaussians start at i0 (a multiple of 64); lanes 0..31 hold the 32 mask
// words of the wave's 1024-block, their popcount prefix plus offsets[block] is the rank of the wave's first selected Gaussian
// (`base`).  The records of the selected Gaussians — the others are not loaded — enter the wave's slots through coalesced 16-byte
// loads, all in flight at once, packed by rank.  Returns the number of selected Gaussians of the wave (wave-uniform).
template <int SH, int STRIDE>
__device__ __forceinline__ uint32_t export_load(const uint4 *__restrict__ src, const uint32_t *__restrict__ words, uint32_t n,
                                                uint32_t invert, const uint32_t *__restrict__ offsets, uint32_t i0, uint32_t lane,
                                                uint4 *slot0, uint64_t &base) {
    constexpr uint32_t SNC = (uint32_t)pod_words(SH, COV_ROT_SCALE) / 4u;      // 16-byte chunks per source record
    uint64_t mask = 0ull;
    base = 0ull;
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
    const uint32_t cnt = (uint32_t)__popcll(mask);
    if (cnt) {
        const uint4 *s = src + (uint64_t)i0 * SNC;
        uint4 v[SNC];
        uint32_t at[SNC];          // where chunk j goes in the wave's slots; ~0: not selected
#pragma unroll
        for (uint32_t j = 0; j < SNC; j++) {
            const uint32_t q = lane + 64u * j;
            const uint32_t r = q / SNC, c = q - r * SNC;            // r < 64: the wave's span is SNC x 64 chunks
            const bool take = (mask >> r) & 1ull;
            at[j] = take ? (uint32_t)__popcll(mask & ((1ull << r) - 1ull)) * (STRIDE / 4) + c : 0xffffffffu;
            v[j] = make_uint4(0u, 0u, 0u, 0u);
            if (take) v[j] = s[q];                                  // a selected record lies below n: its bit passed extract_word
        }
#pragma unroll
        for (uint32_t j = 0; j < SNC; j++)
            if (at[j] != 0xffffffffu) slot0[at[j]] = v[j];
    }
    return cnt;
}

// record `lane` of the wave's slots -> the 56 words of its struct Gaussian (unpack_words), all in registers
template <int SH, int STRIDE>
__device__ __forceinline__ void export_unpack(const uint4 *slot0, uint32_t lane, uint32_t *g) {
    constexpr int SNC = pod_words(SH, COV_ROT_SCALE) / 4;
    const uint4 *rec = slot0 + lane * (STRIDE / 4);
    uint32_t w[SNC * 4];
#pragma unroll
    for (int c = 0; c < SNC; c++) {
        const uint4 v = rec[c];
        w[4 * c] = v.x;
        w[4 * c + 1] = v.y;
        w[4 * c + 2] = v.z;
        w[4 * c + 3] = v.w;
    }
    unpack_words(SH, w, g);
}

// PLY.  One workgroup per 128 source Gaussians from `first` on (a multiple of 1024: the host walks the source in slices of
// whole blocks), one wave per 64.  Lane r turns record r of its wave into the 62 words of a PlyGaussianPod and writes them
// over the record it read (62 <= the 68 words of a slot).  The vertices of a wave are one contiguous span of the output,
// cnt x 62 words from vertex (rank - rank0) of `dst` on — a span that starts on an 8-byte boundary only (248 = 8 x 31), so it
// leaves as 8-byte stores, 31 per vertex, coalesced.  Ranks at or past rank_end are dropped: rank_end - rank0 vertices is what
// `dst` holds, and a selection that another stream changed behind the scan loses records instead of writing past the end.
// LDS: 128 x 68 words = 34 KiB, four workgroups (eight waves) per CU.
constexpr int EXPORT_PLY_STRIDE = export_stride(PLY_WORDS);       // 68
template <int SH>
__global__ __launch_bounds__(EXPORT_GROUP) void k_export_ply(const uint4 *__restrict__ src, uint2 *__restrict__ dst,
                                                             const uint32_t *__restrict__ words, uint32_t n, uint32_t invert,
                                                             const uint32_t *__restrict__ offsets, uint32_t first, uint64_t rank0,
                                                             uint64_t rank_end) {
    constexpr int STRIDE = EXPORT_PLY_STRIDE;
    static_assert(STRIDE >= PLY_WORDS && STRIDE >= pod_words(SH, COV_ROT_SCALE) && STRIDE % 8 == 4, "slot");
    __shared__ uint4 s_rec[EXPORT_GROUP * STRIDE / 4];
    const uint32_t lane = threadIdx.x & 63u, wave0 = threadIdx.x - lane;
    const uint32_t i0 = first + blockIdx.x * EXPORT_GROUP + wave0;
    uint4 *slot0 = s_rec + wave0 * (STRIDE / 4);
    uint64_t base;
    const uint32_t cnt = export_load<SH, STRIDE>(src, words, n, invert, offsets, i0, lane, slot0, base);
    __syncthreads();
    if (lane < cnt) {
        uint32_t g[GAUSSIAN_WORDS], o[64];
        export_unpack<SH, STRIDE>(slot0, lane, g);
        gaussian_to_ply_words(g, o);
        o[62] = 0u;
        o[63] = 0u;
        uint4 *rec = slot0 + lane * (STRIDE / 4);
#pragma unroll
        for (int c = 0; c < 16; c++) rec[c] = make_uint4(o[4 * c], o[4 * c + 1], o[4 * c + 2], o[4 * c + 3]);
    }
    __syncthreads();
    if (cnt && base >= rank0 && base < rank_end) {
        const uint64_t room = rank_end - base;
        const uint32_t keep = room < cnt ? (uint32_t)room : cnt;
        uint2 *d = dst + (base - rank0) * (PLY_WORDS / 2);
        const uint2 *img = (const uint2 *)slot0;
        for (uint32_t q = lane; q < keep * (PLY_WORDS / 2); q += 64u) {
            const uint32_t r = q / (PLY_WORDS / 2), c = q - r * (PLY_WORDS / 2);
            d[q] = img[r * (STRIDE / 2) + c];
        }
    }
}

// where the kernel writes a decompressed SPZ payload: the six columns (device addresses of any alignment), their bytes per
// record, and the options of gaussian_to_spz_bytes
struct SpzOut {
    uint8_t *col[6];
    uint32_t width[6];
    uint32_t version, fractional_bits, ncoef, bucket;
};

// SPZ.  The same front end.  Lane r unpacks record r of its wave to registers; after a barrier (every record of the wave has
// been read) it writes the record's bytes into six column images that reuse the wave's slots: image c holds the wave's entries
// of column c, packed by rank, from byte 64 x (the widths of the columns before c) on.  An image is the wave's span of that
// column, cnt x width bytes from byte rank x width of the column on.  Columns and spans start at any byte, so the 4-byte
// words of the output at the ends of a span are shared with the neighbouring wave or column, which writes them at the same
// time: the bytes of a span in front of the first 4-byte boundary and behind the last one leave as byte stores, the
// words in between — owned by this wave alone — as 4-byte stores, each put together from the two words of the image it
// straddles.  Nothing is read back from the output.  Ranks at or past `total` are dropped.
// LDS: 128 x 60 words = 30 KiB for SH f32 records (36 and 28 words for f16 and snorm8); the images take 64 x 65 bytes of a wave's
// 64 slots.
template <int SH>
__global__ __launch_bounds__(EXPORT_GROUP) void k_export_spz(const uint4 *__restrict__ src, SpzOut out, const uint32_t *__restrict__ words,
                                                             uint32_t n, uint32_t invert, const uint32_t *__restrict__ offsets,
                                                             uint64_t total) {
    constexpr int STRIDE = export_stride(pod_words(SH, COV_ROT_SCALE));
    static_assert(64 * STRIDE * 4 >= 64 * 65 + 4, "the column images of a wave fit its slots");
    __shared__ uint4 s_rec[EXPORT_GROUP * STRIDE / 4];
    const uint32_t lane = threadIdx.x & 63u, wave0 = threadIdx.x - lane;
    const uint32_t i0 = blockIdx.x * EXPORT_GROUP + wave0;
    uint4 *slot0 = s_rec + wave0 * (STRIDE / 4);
    uint64_t base;
    const uint32_t cnt = export_load<SH, STRIDE>(src, words, n, invert, offsets, i0, lane, slot0, base);
    __syncthreads();
    uint32_t g[GAUSSIAN_WORDS];
    if (lane < cnt) export_unpack<SH, STRIDE>(slot0, lane, g);
    __syncthreads();
    uint8_t *img = (uint8_t *)slot0;
    uint32_t img0[6];              // where the image of column c starts: a multiple of 64 bytes
    {
        uint32_t at = 0;
#pragma unroll
        for (int c = 0; c < 6; c++) {
            img0[c] = at;
            at += 64u * out.width[c];
        }
    }
    if (lane < cnt) {
        const uint32_t w0 = out.width[0], w1 = out.width[1], w2 = out.width[2], w3 = out.width[3], w4 = out.width[4], w5 = out.width[5];
        const uint32_t a0 = img0[0] + lane * w0, a1 = img0[1] + lane * w1, a2 = img0[2] + lane * w2, a3 = img0[3] + lane * w3,
                       a4 = img0[4] + lane * w4, a5 = img0[5] + lane * w5;
        gaussian_to_spz_bytes(
            g, out.version, out.fractional_bits, out.ncoef, out.bucket,
            [=](int col, int k, uint32_t byte) {
                const uint32_t a = col == 0 ? a0 : col == 1 ? a1 : col == 2 ? a2 : col == 3 ? a3 : col == 4 ? a4 : a5;
                img[a + (uint32_t)k] = (uint8_t)byte;
            },
            DeviceSqrt());
    }
    __syncthreads();
    if (!cnt || base >= total) return;
    const uint64_t room = total - base;
    const uint32_t keep = room < cnt ? (uint32_t)room : cnt;
#pragma unroll
    for (int c = 0; c < 6; c++) {
        const uint32_t width = out.width[c];
        const uint32_t nbytes = keep * width;
        if (!nbytes) continue;
        uint8_t *d = out.col[c] + base * width;
        const uint8_t *im = img + img0[c];
        const uint32_t *im32 = (const uint32_t *)im;
        uint32_t head = (4u - (uint32_t)((uintptr_t)d & 3u)) & 3u;
        if (head > nbytes) head = nbytes;
        const uint32_t nwords = (nbytes - head) / 4u;
        const uint32_t tail0 = head + 4u * nwords;
        if (lane < head) d[lane] = im[lane];
        if (tail0 + lane < nbytes) d[tail0 + lane] = im[tail0 + lane];
        uint32_t *d32 = (uint32_t *)(d + head);
        for (uint32_t q = lane; q < nwords; q += 64u) {
            const uint32_t l = head + 4u * q;                 // byte of the image where output word q starts
            const uint64_t two = (uint64_t)im32[l >> 2] | ((uint64_t)im32[(l >> 2) + 1u] << 32);
            d32[q] = (uint32_t)(two >> (8u * (l & 3u)));
        }
    }
}

}  // namespace gs
