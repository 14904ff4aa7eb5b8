// gs_deflate_kernels.h — the Huffman-only gzip member on the device.  Included by gs_deflate.hip alone.
// Three kernels and no workgroup waits on another: k_deflate_chunks (one workgroup per 32768-byte chunk: histogram, code,
// bit offsets, the block's image in LDS, its size and CRC), k_deflate_scan (one workgroup: 64-bit byte offsets from the
// sizes) and k_deflate_gather (one workgroup per chunk: the image to its place in the member).  Every format rule is
// gs_deflate.h's, run by one lane; the kernels add only the parallel parts, whose result does not depend on the split.
#pragma once
#include <hip/hip_runtime.h>

#include "gs_deflate.h"

namespace gs {

static __device__ const DfCrcTables k_df_crc = df_make_crc_tables();

// the sum of v over the workgroup's DF_THREADS threads in front of this one, and (total) over all of them
__device__ inline uint32_t df_block_exclusive(uint32_t v, uint32_t *wave_sums, uint32_t &total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = v;
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t up = __shfl_up(inc, d, 64);
        if (lane >= d) inc += up;
    }
    if (lane == 63u) wave_sums[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t w = 0; w < DF_THREADS / 64u; w++) {
        if (w < wave) before += wave_sums[w];
        all += wave_sums[w];
    }
    total = all;
    return before + inc - v;
}

// Chunk blockIdx.x of in[0, len).  sizes[c] = the bytes of its block(s), crcs[c] = the CRC-32 of its input bytes.  With
// `slots` the block is built and written to slots + c DF_SLOT (16-byte aligned); without, only the size is computed.
// The input is read through byte loads: `in` has any alignment.
__global__ __launch_bounds__(DF_THREADS) void k_deflate_chunks(const uint8_t *__restrict__ in, uint64_t len, uint8_t *__restrict__ slots,
                                                               uint32_t *__restrict__ sizes, uint32_t *__restrict__ crcs) {
    __shared__ uint32_t s_img[DF_SLOT / 4u];
    __shared__ uint32_t s_hist[DF_SYMS];
    __shared__ uint32_t s_tab[256];
    __shared__ DfHuff s_h;
    __shared__ uint8_t s_len[DF_SYMS + 3u];
    __shared__ uint16_t s_code[DF_SYMS + 1u];
    __shared__ uint32_t s_wave[DF_THREADS / 64u];
    __shared__ uint32_t s_form, s_hdr_bits, s_bytes, s_crc;

    const uint32_t t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * DF_CHUNK;
    const uint32_t n = (uint32_t)(len - base < DF_CHUNK ? len - base : DF_CHUNK);      // >= 1: the grid is ceil(len / DF_CHUNK)
    const bool final = base + n == len;
    const uint8_t *src = in + base;
    const bool write = slots != nullptr;

    s_hist[t] = 0;
    s_tab[t] = k_df_crc.byte[t];
    if (t == 0) {
        s_hist[DF_EOB] = 1;
        s_crc = 0;
    }
    if (write)
        for (uint32_t i = t; i < DF_SLOT / 4u; i += DF_THREADS) s_img[i] = 0;
    __syncthreads();
    for (uint32_t i = t; i < n; i += DF_THREADS) atomicAdd(&s_hist[src[i]], 1u);
    __syncthreads();

    if (t == 0) {
        const uint32_t b0 = src[0];
        if (n >= 4u && s_hist[b0] == n) {
            s_form = DF_FORM_RUN;
            s_bytes = df_run_block((uint8_t *)s_img, b0, n, final);
        } else {
            uint32_t hdr_bits, bytes;
            s_form = df_plan_chunk(s_hist, n, final, s_len, s_code, (uint8_t *)s_img, s_h, &hdr_bits, &bytes);
            s_hdr_bits = hdr_bits;
            s_bytes = bytes;
        }
    }
    __syncthreads();
    const uint32_t form = s_form, bytes = s_bytes;

    // The pieces are aligned to the END of the chunk: thread t takes the DF_PIECE bytes that end (DF_THREADS - 1 - t) pieces
    // before it, whatever the chunk's length, so the multiplier that carries its CRC to the end is a constant of t.  The
    // threads in front of a short chunk have nothing (an empty piece has CRC 0 and no bits).
    const int32_t e_signed = (int32_t)n - (int32_t)((DF_THREADS - 1u - t) * DF_PIECE);
    const uint32_t end = e_signed > 0 ? (uint32_t)e_signed : 0u;
    const uint32_t start = end > DF_PIECE ? end - DF_PIECE : 0u;
    const bool dynamic = form == DF_FORM_DYNAMIC;
    uint32_t c = 0xffffffffu, nbits = 0;
    for (uint32_t i = start; i < end; i++) {
        const uint32_t b = src[i];
        c = s_tab[(c ^ b) & 255u] ^ (c >> 8);
        if (dynamic) nbits += s_len[b];
    }
    if (end > start) atomicXor(&s_crc, df_crc_mul(~c, k_df_crc.mul[DF_THREADS - 1u - t]));

    if (write && dynamic) {
        uint32_t total;
        const uint32_t first = s_hdr_bits + df_block_exclusive(nbits, s_wave, total);
        // codes go into a 64-bit window whose low bits are those of the word where the thread begins; whole words are OR-ed
        // into the zeroed image (the first and the last one are shared with the neighbours, and with the header)
        uint32_t word = first >> 5, fill = first & 31u;
        uint64_t acc = 0;
        for (uint32_t i = start; i < end; i++) {
            const uint32_t b = src[i];
            acc |= (uint64_t)s_code[b] << fill;
            fill += s_len[b];
            if (fill >= 32u) {
                atomicOr(&s_img[word++], (uint32_t)acc);
                acc >>= 32;
                fill -= 32u;
            }
        }
        if (t == DF_THREADS - 1u) {      // the last piece is never empty: end of block, and what closes the block
            acc |= (uint64_t)s_code[DF_EOB] << fill;
            fill += s_len[DF_EOB];
            if (fill >= 32u) {
                atomicOr(&s_img[word++], (uint32_t)acc);
                acc >>= 32;
                fill -= 32u;
            }
            if (!final) {      // 000, the pad and 00 00 are the zeroes of the image; ff ff are its last two bytes
                const uint32_t at = bytes - 2u;
                atomicOr(&s_img[at >> 2], 0xffu << (8u * (at & 3u)));
                atomicOr(&s_img[(at + 1u) >> 2], 0xffu << (8u * ((at + 1u) & 3u)));
            }
        }
        if (fill) atomicOr(&s_img[word], (uint32_t)acc);
    }
    __syncthreads();

    if (write) {
        uint8_t *slot = slots + (uint64_t)blockIdx.x * DF_SLOT;
        if (form == DF_FORM_STORED) {
            if (t == 0) df_stored_header(slot, n, final);
            for (uint32_t i = t; i < n; i += DF_THREADS) slot[5u + i] = src[i];
        } else {
            uint32_t *slot32 = (uint32_t *)slot;      // bytes <= DF_CHUNK + 4: the words stay inside the slot
            for (uint32_t i = t; i < (bytes + 3u) / 4u; i += DF_THREADS) slot32[i] = s_img[i];
        }
    }
    if (t == 0) {
        sizes[blockIdx.x] = bytes;
        crcs[blockIdx.x] = s_crc;
    }
}

// offsets[c] = the sum of sizes[0, c), offsets[n] = the size of the stream: one workgroup, each thread a run of chunks
__global__ __launch_bounds__(DF_THREADS) void k_deflate_scan(const uint32_t *__restrict__ sizes, uint64_t *__restrict__ offsets, uint32_t n) {
    __shared__ uint64_t s_sum[DF_THREADS];
    const uint32_t t = threadIdx.x, per = (n + DF_THREADS - 1u) / DF_THREADS;
    const uint32_t a = t * per < n ? t * per : n, b = a + per < n ? a + per : n;
    uint64_t sum = 0;
    for (uint32_t i = a; i < b; i++) sum += sizes[i];
    s_sum[t] = sum;
    __syncthreads();
    uint64_t at = 0;
    for (uint32_t k = 0; k < t; k++) at += s_sum[k];
    for (uint32_t i = a; i < b; i++) {
        offsets[i] = at;
        at += sizes[i];
    }
    if (t == DF_THREADS - 1u) offsets[n] = at;
}

// the image of chunk blockIdx.x to body + offsets[c]: aligned words of the member, each from four bytes of the slot
__global__ __launch_bounds__(DF_THREADS) void k_deflate_gather(const uint8_t *__restrict__ slots, const uint32_t *__restrict__ sizes,
                                                               const uint64_t *__restrict__ offsets, uint8_t *__restrict__ body) {
    const uint32_t t = threadIdx.x, size = sizes[blockIdx.x];
    const uint8_t *src = slots + (uint64_t)blockIdx.x * DF_SLOT;
    uint8_t *dst = body + offsets[blockIdx.x];
    uint32_t head = (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u);
    if (head > size) head = size;
    const uint32_t words = (size - head) / 4u, tail = head + 4u * words;
    if (t < head) dst[t] = src[t];
    for (uint32_t w = t; w < words; w += DF_THREADS) {
        const uint32_t o = head + 4u * w;
        *(uint32_t *)(dst + o) = (uint32_t)src[o] | (uint32_t)src[o + 1u] << 8 | (uint32_t)src[o + 2u] << 16 | (uint32_t)src[o + 3u] << 24;
    }
    if (tail + t < size) dst[tail + t] = src[tail + t];
}

}  // namespace gs
