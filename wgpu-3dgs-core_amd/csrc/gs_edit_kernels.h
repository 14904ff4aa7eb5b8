// gs_edit_kernels.h — edits of the selected Gaussians in place, their extraction into a new buffer (include/gs3d.h
// gs_gaussians_buffer_edit / _create_from_selection) and snapshots of them (_snapshot / _restore; §3.9).  No reference item: the reference's editor does
// this with compute passes over the Gaussian buffer; the core crate has none.
//
// The codecs are the library's own: records are decoded with gs_kernel_lib.h (gaussian_unpack_sh / _cov3d, unorm8) and
// re-encoded with gs_device_common.h / gs_convert.h (f32_to_f16_rtne_bits, sh_norm8_byte, cv_sat_u8, cv_canon_nan_bits).
#pragma once

#include "gs_convert.h"
#include "gs_device_common.h"

namespace gs {

enum : uint32_t { EDIT_TRANSFORM = 1u, EDIT_ROTATE_SH = 2u, EDIT_COLOR = 4u, EDIT_OPACITY = 8u };

// the constants of one edit, computed on the host (512 bytes of kernel argument)
struct EditArgs {
    float M[16];      // model_transform_mat(transform), column-major 4 x 4
    float A[9];       // model_scale_rot_mat(transform), column-major 3 x 3
    float q[4];       // transform.rot, xyzw, as given
    float s;          // transform.scale.x
    float D1[9], D2[25], D3[49];   // gs_sh_rotation_matrices, row-major
    float C[12];      // colour, column-major 3 x 4
    float o[2];       // opacity: a' = o[0] a + o[1]
    uint32_t flags;
};

__device__ __forceinline__ uint32_t edit_unorm_byte(float v) { return cv_sat_u8(v * 255.0f + 0.5f); }

// rgb' = ((C0 r + C3 g) + C6 b) [+ C9]
__device__ __forceinline__ vec3 edit_color_linear(const float *C, vec3 v) {
    return {(C[0] * v.x + C[3] * v.y) + C[6] * v.z, (C[1] * v.x + C[4] * v.y) + C[7] * v.z,
            (C[2] * v.x + C[5] * v.y) + C[8] * v.z};
}

// one band of the SH rotation: out_k = sum_j D[k][j] in_j, summed in j order, per channel
template <int NB>
__device__ __forceinline__ void edit_rotate_band(const float *D, vec3 *c) {
    vec3 out[NB];
#pragma unroll
    for (int k = 0; k < NB; k++) {
        vec3 a = {D[k * NB] * c[0].x, D[k * NB] * c[0].y, D[k * NB] * c[0].z};
#pragma unroll
        for (int j = 1; j < NB; j++) {
            a.x = a.x + D[k * NB + j] * c[j].x;
            a.y = a.y + D[k * NB + j] * c[j].y;
            a.z = a.z + D[k * NB + j] * c[j].z;
        }
        out[k] = a;
    }
#pragma unroll
    for (int k = 0; k < NB; k++) c[k] = out[k];
}

// 45 f32 rest coefficients -> the layout's SH words (the arithmetic of pack_words)
template <int SH>
__device__ __forceinline__ void edit_encode_sh(const vec3 *c, uint32_t *s) {
    uint32_t bits[45];
#pragma unroll
    for (int k = 0; k < 15; k++) {
        bits[3 * k] = cv_canon_nan_bits(c[k].x);
        bits[3 * k + 1] = cv_canon_nan_bits(c[k].y);
        bits[3 * k + 2] = cv_canon_nan_bits(c[k].z);
    }
    if constexpr (SH == SH_SINGLE) {
#pragma unroll
        for (int k = 0; k < 45; k++) s[k] = bits[k];
    } else if constexpr (SH == SH_HALF) {
#pragma unroll
        for (int k = 0; k < 23; k++) s[k] = 0u;
#pragma unroll
        for (int k = 0; k < 45; k++) s[k >> 1] |= (uint32_t)f32_to_f16_rtne_bits(bits[k]) << (16 * (k & 1));
    } else if constexpr (SH == SH_NORM8) {
#pragma unroll
        for (int k = 0; k < 12; k++) s[k] = 0u;
#pragma unroll
        for (int k = 0; k < 45; k++) s[k >> 2] |= sh_norm8_byte(u2f(bits[k])) << (8 * (k & 3));
    }
}

// One thread per Gaussian of the AoS buffer.  A wave whose 64 selection bits are all 0 returns after reading its two
// words; a selected record is loaded and stored as 16-byte vectors.
template <int SH, int COV>
__global__ __launch_bounds__(256) void k_edit(uint4 *__restrict__ aos, uint32_t n, const uint32_t *__restrict__ words,
                                              EditArgs e) {
    constexpr int NC = pod_bytes(SH, COV) / 16, NW = NC * 4;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    const uint64_t mask = wave_selection_mask(words, i - lane, n);
    if (mask == 0ull) return;
    if (!((mask >> lane) & 1ull)) return;      // (bits at positions >= n are never set)
    uint4 *rec = aos + (uint64_t)i * NC;
    uint32_t w[NW];
#pragma unroll
    for (int c = 0; c < NC; c++) {
        const uint4 v = rec[c];
        w[4 * c] = v.x;
        w[4 * c + 1] = v.y;
        w[4 * c + 2] = v.z;
        w[4 * c + 3] = v.w;
    }
    uint32_t *cw = w + cov_word0(SH);
    if (e.flags & EDIT_TRANSFORM) {
        const float p[3] = {u2f(w[0]), u2f(w[1]), u2f(w[2])};
        float pw[4];
        mat4_mul_point(e.M, p, pw);
#pragma unroll
        for (int k = 0; k < 3; k++) w[k] = cv_canon_nan_bits(pw[k]);
        if constexpr (COV == COV_ROT_SCALE) {
            const float rx = u2f(cw[0]), ry = u2f(cw[1]), rz = u2f(cw[2]), rw = u2f(cw[3]);
            const float qx = e.q[0], qy = e.q[1], qz = e.q[2], qw = e.q[3];
            cw[0] = cv_canon_nan_bits(((qw * rx + qx * rw) + qy * rz) - qz * ry);
            cw[1] = cv_canon_nan_bits(((qw * ry - qx * rz) + qy * rw) + qz * rx);
            cw[2] = cv_canon_nan_bits(((qw * rz + qx * ry) - qy * rx) + qz * rw);
            cw[3] = cv_canon_nan_bits(((qw * rw - qx * rx) - qy * ry) - qz * rz);
#pragma unroll
            for (int k = 0; k < 3; k++) cw[4 + k] = cv_canon_nan_bits(e.s * u2f(cw[4 + k]));
        } else {
            float c6[6];
            gaussian_unpack_cov3d<SH, COV>(w, c6);
            const float S[3][3] = {{c6[0], c6[1], c6[2]}, {c6[1], c6[3], c6[4]}, {c6[2], c6[4], c6[5]}};
            float T[3][3];      // T = A Sigma; A[r][k] = e.A[3 k + r]
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = 0; c < 3; c++) T[r][c] = (e.A[r] * S[0][c] + e.A[3 + r] * S[1][c]) + e.A[6 + r] * S[2][c];
#define GS_EDIT_SIG(r, c) cv_canon_nan_bits((T[r][0] * e.A[c] + T[r][1] * e.A[3 + c]) + T[r][2] * e.A[6 + c])
            const uint32_t o[6] = {GS_EDIT_SIG(0, 0), GS_EDIT_SIG(0, 1), GS_EDIT_SIG(0, 2),
                                   GS_EDIT_SIG(1, 1), GS_EDIT_SIG(1, 2), GS_EDIT_SIG(2, 2)};
#undef GS_EDIT_SIG
            if constexpr (COV == COV_SINGLE) {
#pragma unroll
                for (int k = 0; k < 6; k++) cw[k] = o[k];
            } else {
#pragma unroll
                for (int k = 0; k < 3; k++)
                    cw[k] = (uint32_t)f32_to_f16_rtne_bits(o[2 * k]) | ((uint32_t)f32_to_f16_rtne_bits(o[2 * k + 1]) << 16);
            }
        }
    }
    if constexpr (SH != SH_NONE) {
        if (e.flags & (EDIT_ROTATE_SH | EDIT_COLOR)) {
            vec3 c[15];
#pragma unroll
            for (int k = 0; k < 15; k++) c[k] = gaussian_unpack_sh<SH>(w, (uint32_t)k);
            if (e.flags & EDIT_ROTATE_SH) {
                edit_rotate_band<3>(e.D1, c);
                edit_rotate_band<5>(e.D2, c + 3);
                edit_rotate_band<7>(e.D3, c + 8);
            }
            if (e.flags & EDIT_COLOR) {
#pragma unroll
                for (int k = 0; k < 15; k++) c[k] = edit_color_linear(e.C, c[k]);
            }
            edit_encode_sh<SH>(c, w + sh_word0(SH));
        }
    }
    uint32_t col = w[3];
    if (e.flags & EDIT_COLOR) {
        const vec3 l = edit_color_linear(e.C, {unorm8(col, 0), unorm8(col, 1), unorm8(col, 2)});
        col = (col & 0xff000000u) | edit_unorm_byte(l.x + e.C[9]) | (edit_unorm_byte(l.y + e.C[10]) << 8) |
              (edit_unorm_byte(l.z + e.C[11]) << 16);
    }
    if (e.flags & EDIT_OPACITY)
        col = (col & 0x00ffffffu) | (edit_unorm_byte(e.o[0] * unorm8(col, 3) + e.o[1]) << 24);
    w[3] = col;
#pragma unroll
    for (int c = 0; c < NC; c++) rec[c] = make_uint4(w[4 * c], w[4 * c + 1], w[4 * c + 2], w[4 * c + 3]);
}

// ---- extraction: per-block counts -> k_scan_chunks -> stable copy ------------------------------------------------

// (extract_word, the mask word that an extraction copies: gs_device_common.h — the relayout unit locates records with it too)

// counts[b] = selected Gaussians of the 1024-Gaussian block b (32 mask words): one thread per word, summed over the 32
// lanes of a wave half.  nblocks * 32 threads do work; the grid is rounded up to whole workgroups.
__global__ __launch_bounds__(256) void k_extract_block_counts(const uint32_t *__restrict__ words, uint32_t n, uint32_t invert,
                                                              uint32_t nblocks, uint32_t *__restrict__ counts) {
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    uint32_t c = (uint32_t)__popc(extract_word(words, w, n, invert));
#pragma unroll
    for (int d = 16; d >= 1; d >>= 1) c += (uint32_t)__shfl_xor((int)c, d, 32);
    if ((threadIdx.x & 31u) == 0u && (w >> 5) < nblocks) counts[w >> 5] = c;
}

// One wave per 64 source Gaussians.  Lanes 0..31 hold the 32 mask words of the wave's 1024-block; their popcount prefix
// gives the rank of the wave's first Gaussian inside the block, offsets[block] (k_scan_chunks) the block's first
// destination.  The wave's 64 records are one contiguous span of 64 x nc 16-byte chunks, and those of its selected
// Gaussians are contiguous in the destination too: lane after lane takes chunk after chunk.  Destination order = caller
// order (stable).  `total` is the destination's length: a selection that another stream changed behind the count (the
// caller's error) loses records instead of writing past the end.
__global__ __launch_bounds__(256) void k_extract_copy(const uint4 *__restrict__ src, uint4 *__restrict__ dst,
                                                      const uint32_t *__restrict__ words, uint32_t n, uint32_t invert,
                                                      const uint32_t *__restrict__ offsets, uint32_t nc, uint32_t total) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t i0 = blockIdx.x * 256u + (threadIdx.x - lane);      // first Gaussian of the wave
    if (i0 >= n) return;
    const uint32_t block = i0 / PLANAR_BLOCK, wsel = (i0 % PLANAR_BLOCK) >> 5;     // the wave's first word inside the block
    const uint32_t word = lane < 32u ? extract_word(words, block * 32u + lane, n, invert) : 0u;
    const uint32_t pc = (uint32_t)__popc(word);
    const uint32_t inc = wave_inclusive_scan(pc, lane);
    const uint32_t lo = (uint32_t)__shfl((int)word, (int)wsel), hi = (uint32_t)__shfl((int)word, (int)wsel + 1);
    const uint32_t before = (uint32_t)__shfl((int)(inc - pc), (int)wsel);
    const uint64_t mask = (uint64_t)lo | ((uint64_t)hi << 32);
    if (mask == 0ull) return;
    const uint64_t base = (uint64_t)offsets[block] + before;
    const uint4 *s = src + (uint64_t)i0 * nc;
    for (uint32_t q = lane; q < 64u * nc; q += 64u) {
        const uint32_t r = q / nc, c = q - r * nc;
        if (!((mask >> r) & 1ull)) continue;
        const uint32_t rank = (uint32_t)__popcll(mask & ((1ull << r) - 1ull));
        if (base + rank < total) dst[(base + rank) * nc + c] = s[q];
    }
}

// ---- snapshots of the selected records (gs_gaussians_buffer_snapshot / _restore) -------------------

// the mask a snapshot keeps: the selection's words (null: all), bits >= n cleared
__global__ __launch_bounds__(256) void k_snapshot_mask(uint32_t *__restrict__ dst, const uint32_t *__restrict__ words,
                                                       uint32_t nwords, uint32_t n) {
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w < nwords) dst[w] = extract_word(words, w, n, 0u);
}

// The reverse of k_extract_copy: one wave per 64 target Gaussians.  Lanes 0..31 hold the 32 words of the SNAPSHOT'S mask
// for the wave's 1024-block; their popcount prefix plus offsets[block] (kept from the snapshot's scan) is the rank of the
// wave's first record in the snapshot.  The records of the wave's selected Gaussians are contiguous on both sides: lane
// after lane takes chunk after chunk.  EXCHANGE: the buffer gets the snapshot's chunk and the snapshot what the buffer
// held; a lane loads both before it stores either.  A wave without a selected Gaussian returns after reading its words.
// `count` is the snapshot's length: nothing past it is read or written.
template <bool EXCHANGE>
__global__ __launch_bounds__(256) void k_restore(uint4 *__restrict__ aos, uint4 *__restrict__ snap,
                                                 const uint32_t *__restrict__ words, uint32_t n,
                                                 const uint32_t *__restrict__ offsets, uint32_t nc, uint32_t count) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t i0 = blockIdx.x * 256u + (threadIdx.x - lane);      // first Gaussian of the wave
    if (i0 >= n) return;
    const uint32_t block = i0 / PLANAR_BLOCK, wsel = (i0 % PLANAR_BLOCK) >> 5;
    const uint32_t word = lane < 32u ? extract_word(words, block * 32u + lane, n, 0u) : 0u;
    const uint32_t pc = (uint32_t)__popc(word);
    const uint32_t inc = wave_inclusive_scan(pc, lane);
    const uint32_t lo = (uint32_t)__shfl((int)word, (int)wsel), hi = (uint32_t)__shfl((int)word, (int)wsel + 1);
    const uint32_t before = (uint32_t)__shfl((int)(inc - pc), (int)wsel);
    const uint64_t mask = (uint64_t)lo | ((uint64_t)hi << 32);
    if (mask == 0ull) return;
    const uint64_t base = (uint64_t)offsets[block] + before;
    uint4 *t = aos + (uint64_t)i0 * nc;
    for (uint32_t q = lane; q < 64u * nc; q += 64u) {
        const uint32_t r = q / nc, c = q - r * nc;
        if (!((mask >> r) & 1ull)) continue;
        const uint64_t rank = base + (uint32_t)__popcll(mask & ((1ull << r) - 1ull));
        if (rank >= count) continue;
        uint4 *sp = snap + rank * nc + c;
        const uint4 v = *sp;
        if constexpr (EXCHANGE) {
            const uint4 old = t[q];
            *sp = old;
        }
        t[q] = v;
    }
}

}  // namespace gs
