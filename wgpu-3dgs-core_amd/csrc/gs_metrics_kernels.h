// gs_metrics_kernels.h — image metrics (include/gs3d.h gs_image_compare): per-channel error sums, maxima and
// counts of two H x W x 4 binary32 images, the 11 x 11 Gaussian-window SSIM of their colour channels, and the two optional
// per-pixel planes.  No reference item: the reference compares nothing on the device.
//
// Every binary32 operation is rounded (-ffp-contract=off) and written in the order DESIGN.md §3.14 fixes; the division is the
// correctly rounded one.  The sums are binary64, folded in a shape that depends on the grid alone: wave butterfly
// (gs_stats_kernels.h has the same one for its unit), the four waves in wave order, one partial row per workgroup,
// k_metrics_finish.  No floating-point atomics.
#pragma once

#include "gs_device_common.h"

namespace gs {

// exp(-(k - 5)^2 / 4.5) / sum, k = 0..10, rounded to binary32 (tests/metrics_np.py derives the same bits)
__device__ constexpr float SSIM_G[11] = {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c4p-3f, 0x1.10656p-2f,
                                         0x1.b43c4p-3f,   0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f};

constexpr int MET_TW = 32, MET_TH = 16, MET_R = 5;                            // tile, window radius
constexpr int MET_RW = MET_TW + 2 * MET_R, MET_RH = MET_TH + 2 * MET_R;      // the tile with its halo: 42 x 26
constexpr int MET_HALO = MET_RW * MET_RH - MET_TW * MET_TH;                  // pixels of the halo alone: 580
constexpr int MET_HSLOTS = (MET_HALO + 255) / 256;                           // ... per thread: 3
// workgroups = partial rows of one call: eight per CU of the MI355X, so that a large image gives every workgroup several
// tiles to spread its one reduction over
constexpr uint32_t MET_MAX_GROUPS = 2048u;

// One partial row per workgroup, field-major (part[f * nblocks + block]).
// part_d: 0..3 sum_sq, 4..7 sum_abs, 8..10 ssim_sum.  part_k: 0..3 the max keys.  part_u: finite, differing, bit_differing,
// ssim_finite r g b.
constexpr uint32_t MET_D_FIELDS = 11u, MET_K_FIELDS = 4u, MET_U_FIELDS = 6u;

// what k_metrics_finish leaves on the device: the layout of gs_image_metrics (include/gs3d.h)
struct MetricsOut {
    uint64_t pixels, finite, differing, bit_differing;
    double sum_sq[4], sum_abs[4];
    float max_abs[4];
    uint32_t max_abs_at[4];
    double ssim_sum[3];
    uint64_t ssim_finite[3];
};

// the running values of one thread
struct MetricsAcc {
    double d[MET_D_FIELDS];
    uint64_t k[MET_K_FIELDS];      // (bits of |d_c|) << 32 | ~index: the largest key is the largest value at its smallest index
    uint32_t u[MET_U_FIELDS];
};

__device__ __forceinline__ void metrics_acc_init(MetricsAcc &m) {
#pragma unroll
    for (int f = 0; f < (int)MET_D_FIELDS; f++) m.d[f] = 0.0;
#pragma unroll
    for (int f = 0; f < (int)MET_K_FIELDS; f++) m.k[f] = 0ull;
#pragma unroll
    for (int f = 0; f < (int)MET_U_FIELDS; f++) m.u[f] = 0u;
}

// the error fields of pixel `p`, and its value of the error plane
__device__ __forceinline__ float metrics_pixel(MetricsAcc &m, const float4 &a, const float4 &b, uint32_t p) {
    const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
    bool fin = true, bits = false;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        fin = fin && attr_finite(av[c]) && attr_finite(bv[c]);
        bits = bits || f2u(av[c]) != f2u(bv[c]);
    }
    m.u[2] += bits ? 1u : 0u;
    if (!fin) return u2f(0x7fc00000u);
    m.u[0] += 1u;
    bool differs = false;
    float e = 0.0f;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const float d = av[c] - bv[c], ad = fabsf(d);      // finite inputs: d is finite or an infinity, never NaN
        differs = differs || d != 0.0f;
        m.d[c] = m.d[c] + (double)d * (double)d;
        m.d[4 + c] = m.d[4 + c] + (double)ad;
        const uint64_t key = ((uint64_t)f2u(ad) << 32) | (uint64_t)(~p);
        m.k[c] = key > m.k[c] ? key : m.k[c];
        e = c == 0 ? ad : fmaxf(e, ad);
    }
    m.u[1] += differs ? 1u : 0u;
    return e;
}

__device__ __forceinline__ uint64_t wave_reduce_max64(uint64_t v) {
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1) {
        const uint64_t o = __shfl_xor((unsigned long long)v, d, WAVE);
        v = o > v ? o : v;
    }
    return v;
}
// wave sum of a double in a fixed shape (a butterfly: both partners of a step add the same two values); all 64 lanes active
__device__ __forceinline__ double metrics_wave_add_f64(double v) {
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1) v = v + __shfl_xor(v, d, WAVE);
    return v;
}

struct MetricsShared {
    double d[4][MET_D_FIELDS];
    uint64_t k[4][MET_K_FIELDS];
    uint32_t u[4][MET_U_FIELDS];
};

// the workgroup's row: wave reductions, then the four waves through LDS in wave order.  All 256 threads call it.
template <bool SSIM>
__device__ __forceinline__ void metrics_write_row(MetricsAcc &m, MetricsShared &sh, double *__restrict__ part_d,
                                                  unsigned long long *__restrict__ part_k, uint32_t *__restrict__ part_u,
                                                  uint32_t nblocks) {
    constexpr int ND = SSIM ? (int)MET_D_FIELDS : 8, NU = SSIM ? (int)MET_U_FIELDS : 3;
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
#pragma unroll
    for (int f = 0; f < ND; f++) m.d[f] = metrics_wave_add_f64(m.d[f]);
#pragma unroll
    for (int f = 0; f < (int)MET_K_FIELDS; f++) m.k[f] = wave_reduce_max64(m.k[f]);
#pragma unroll
    for (int f = 0; f < NU; f++) m.u[f] = wave_reduce_add(m.u[f]);
    if (lane == 0u) {
#pragma unroll
        for (int f = 0; f < (int)MET_D_FIELDS; f++) sh.d[wid][f] = f < ND ? m.d[f] : 0.0;
#pragma unroll
        for (int f = 0; f < (int)MET_K_FIELDS; f++) sh.k[wid][f] = m.k[f];
#pragma unroll
        for (int f = 0; f < (int)MET_U_FIELDS; f++) sh.u[wid][f] = f < NU ? m.u[f] : 0u;
    }
    __syncthreads();
    const uint32_t f = threadIdx.x;
    if (f < MET_D_FIELDS) {
        part_d[(uint64_t)f * nblocks + blockIdx.x] = (sh.d[0][f] + sh.d[1][f]) + (sh.d[2][f] + sh.d[3][f]);
    } else if (f >= 64u && f < 64u + MET_K_FIELDS) {
        const uint32_t g = f - 64u;
        const uint64_t x0 = sh.k[0][g], x1 = sh.k[1][g], x2 = sh.k[2][g], x3 = sh.k[3][g];
        const uint64_t m01 = x0 > x1 ? x0 : x1, m23 = x2 > x3 ? x2 : x3;
        part_k[(uint64_t)g * nblocks + blockIdx.x] = m01 > m23 ? m01 : m23;
    } else if (f >= 128u && f < 128u + MET_U_FIELDS) {
        const uint32_t g = f - 128u;
        part_u[(uint64_t)g * nblocks + blockIdx.x] = (sh.u[0][g] + sh.u[1][g]) + (sh.u[2][g] + sh.u[3][g]);
    }
}

// ---- pass 1 ----------------------------------------------------------------------------------------------------------

__device__ __forceinline__ float metrics_channel(const float4 &v, int c) { return c == 0 ? v.x : c == 1 ? v.y : v.z; }

// the per-pixel SSIM value from the five filtered planes
__device__ __forceinline__ float ssim_value(float ma, float mb, float eaa, float eab, float ebb, float C1, float C2) {
    const float maa = ma * ma, mbb = mb * mb, mab = ma * mb;
    const float saa = eaa - maa, sbb = ebb - mbb, sab = eab - mab;
    return ((2.0f * mab + C1) * (2.0f * sab + C2)) / (((maa + mbb) + C1) * ((saa + sbb) + C2));
}

// pixel e of the 580 of the halo alone, in the halo tile's coordinates: the five rows above the tile, the five below, then the
// ten columns beside each of its sixteen rows
__device__ __forceinline__ void metrics_halo_slot(int e, int &ry, int &rx) {
    if (e < 2 * MET_R * MET_RW) {
        const int r = e / MET_RW;
        rx = e - r * MET_RW;
        ry = r < MET_R ? r : r + MET_TH;
    } else {
        const int f = e - 2 * MET_R * MET_RW, r = f / (2 * MET_R), c = f - r * (2 * MET_R);
        ry = MET_R + r;
        rx = c < MET_R ? c : c + MET_TW;
    }
}

// One workgroup takes the tiles blockIdx.x, blockIdx.x + gridDim.x, ... (32 x 16 pixels each); thread t owns the pixels of
// column t % 32 in rows t / 32 and t / 32 + 8.  It loads them as float4 (a half-wave reads 512 consecutive bytes of a row),
// adds them to its error fields and writes the error plane.  That is all the instantiation without SSIM does: each image is
// read exactly once, no halo, no LDS beyond the reduction; and since both instantiations visit the pixels in the same
// order on the same grid, the error fields of a call do not depend on the flag.
// With SSIM the 580 pixels of the 5-pixel halo are loaded too, up to three per thread; all five pairs stay in registers and
// pixels outside the image are +0.  Then, one colour channel at a time: the channel of both images goes into two planar LDS
// tiles (42 x 26), the horizontal pass writes the five filtered planes (a, b, a a, a b, b b; 26 rows x 32 columns each),
// the vertical pass reads them.  In both passes the 32 lanes of a half-wave read 32 consecutive words of one row:
// conflict-free.  LDS: 2 x 4368 + 5 x 3328 = 25376 bytes plus the reduction's 576.
template <bool SSIM>
__global__ __launch_bounds__(256) void k_metrics_tiles(const float4 *__restrict__ a, const float4 *__restrict__ b, uint32_t width,
                                                       uint32_t height, uint32_t tiles_x, uint32_t ntiles, float C1, float C2,
                                                       float *__restrict__ err_plane, float *__restrict__ ssim_plane,
                                                       double *__restrict__ part_d, unsigned long long *__restrict__ part_k,
                                                       uint32_t *__restrict__ part_u, uint32_t nblocks) {
    __shared__ float s_a[SSIM ? MET_RH : 1][MET_RW], s_b[SSIM ? MET_RH : 1][MET_RW];
    __shared__ float s_h[SSIM ? 5 : 1][SSIM ? MET_RH : 1][MET_TW];
    __shared__ MetricsShared sh;
    MetricsAcc m;
    metrics_acc_init(m);
    const uint32_t tid = threadIdx.x;
    const int tx = (int)(tid & 31u), ty = (int)(tid >> 5);
    for (uint32_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t x0 = (int64_t)(t % tiles_x) * MET_TW, y0 = (int64_t)(t / tiles_x) * MET_TH;
        // 1. the thread's own two pixels
        float4 va[2], vb[2];
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const int64_t x = x0 + tx, y = y0 + ty + 8 * q;
            va[q] = vb[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (x < (int64_t)width && y < (int64_t)height) {
                const uint64_t p = (uint64_t)y * width + (uint64_t)x;
                va[q] = a[p];
                vb[q] = b[p];
                const float e = metrics_pixel(m, va[q], vb[q], (uint32_t)p);
                if (err_plane) err_plane[p] = e;
            }
        }
        if constexpr (SSIM) {
            // 2. its share of the halo
            float4 ha[MET_HSLOTS], hb[MET_HSLOTS];
#pragma unroll
            for (int j = 0; j < MET_HSLOTS; j++) {
                const int e = (int)tid + 256 * j;
                int ry = 0, rx = 0;
                metrics_halo_slot(e, ry, rx);
                const int64_t x = x0 + rx - MET_R, y = y0 + ry - MET_R;
                ha[j] = hb[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (e < MET_HALO && x >= 0 && y >= 0 && x < (int64_t)width && y < (int64_t)height) {
                    const uint64_t p = (uint64_t)y * width + (uint64_t)x;
                    ha[j] = a[p];
                    hb[j] = b[p];
                }
            }
            float sv[2][3];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                // 3. the channel, planar (the barrier also ends the previous channel's / tile's reads)
                __syncthreads();
#pragma unroll
                for (int q = 0; q < 2; q++) {
                    s_a[MET_R + ty + 8 * q][MET_R + tx] = metrics_channel(va[q], c);
                    s_b[MET_R + ty + 8 * q][MET_R + tx] = metrics_channel(vb[q], c);
                }
#pragma unroll
                for (int j = 0; j < MET_HSLOTS; j++) {
                    const int e = (int)tid + 256 * j;
                    int ry = 0, rx = 0;
                    metrics_halo_slot(e, ry, rx);
                    if (e < MET_HALO) {
                        s_a[ry][rx] = metrics_channel(ha[j], c);
                        s_b[ry][rx] = metrics_channel(hb[j], c);
                    }
                }
                __syncthreads();
                // 4. horizontal: 26 rows x 32 columns
                for (int i = (int)tid; i < MET_RH * MET_TW; i += 256) {
                    const int ry = i >> 5, cx = i & 31;
                    float fa = 0.0f, fb = 0.0f, faa = 0.0f, fab = 0.0f, fbb = 0.0f;
#pragma unroll
                    for (int k = 0; k < 11; k++) {
                        const float pa = s_a[ry][cx + k], pb = s_b[ry][cx + k], g = SSIM_G[k];
                        const float paa = pa * pa, pab = pa * pb, pbb = pb * pb;
                        fa = fa + g * pa;
                        fb = fb + g * pb;
                        faa = faa + g * paa;
                        fab = fab + g * pab;
                        fbb = fbb + g * pbb;
                    }
                    s_h[0][ry][cx] = fa;
                    s_h[1][ry][cx] = fb;
                    s_h[2][ry][cx] = faa;
                    s_h[3][ry][cx] = fab;
                    s_h[4][ry][cx] = fbb;
                }
                __syncthreads();
                // 5. vertical and the value
#pragma unroll
                for (int q = 0; q < 2; q++) {
                    const int py = ty + 8 * q;
                    float f[5];
#pragma unroll
                    for (int pl = 0; pl < 5; pl++) {
                        float acc = 0.0f;
#pragma unroll
                        for (int k = 0; k < 11; k++) acc = acc + SSIM_G[k] * s_h[pl][py + k][tx];
                        f[pl] = acc;
                    }
                    const float s = ssim_value(f[0], f[1], f[2], f[3], f[4], C1, C2);
                    sv[q][c] = s;
                    if (x0 + tx < (int64_t)width && y0 + py < (int64_t)height && attr_finite(s)) {
                        m.d[8 + c] = m.d[8 + c] + (double)s;
                        m.u[3 + c] += 1u;
                    }
                }
            }
            if (ssim_plane) {
#pragma unroll
                for (int q = 0; q < 2; q++) {
                    const int64_t x = x0 + tx, y = y0 + ty + 8 * q;
                    if (x < (int64_t)width && y < (int64_t)height)
                        ssim_plane[(uint64_t)y * width + (uint64_t)x] = ((sv[q][0] + sv[q][1]) + sv[q][2]) / 3.0f;
                }
            }
        }
    }
    metrics_write_row<SSIM>(m, sh, part_d, part_k, part_u, nblocks);
}

// ---- pass 2 ----------------------------------------------------------------------------------------------------------

// One workgroup.  Thread t takes the partial rows t, t + 256, ... in ascending order; the 256 running values are reduced
// across the wave and then across the four waves in wave order.  The shape depends on nblocks alone, so the sums are the
// same bits from run to run.  `pixels` is the host's.
__global__ __launch_bounds__(256) void k_metrics_finish(const double *__restrict__ part_d, const unsigned long long *__restrict__ part_k,
                                                        const uint32_t *__restrict__ part_u, uint32_t nblocks, uint64_t pixels,
                                                        MetricsOut *__restrict__ out) {
    __shared__ double s_d[4][MET_D_FIELDS];
    __shared__ uint64_t s_k[4][MET_K_FIELDS];
    __shared__ uint64_t s_c[4][MET_U_FIELDS];
    const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
    double d[MET_D_FIELDS];
    uint64_t k[MET_K_FIELDS], c[MET_U_FIELDS];
#pragma unroll
    for (int f = 0; f < (int)MET_D_FIELDS; f++) d[f] = 0.0;
#pragma unroll
    for (int f = 0; f < (int)MET_K_FIELDS; f++) k[f] = 0ull;
#pragma unroll
    for (int f = 0; f < (int)MET_U_FIELDS; f++) c[f] = 0ull;
    for (uint32_t b = threadIdx.x; b < nblocks; b += 256u) {
#pragma unroll
        for (int f = 0; f < (int)MET_D_FIELDS; f++) d[f] = d[f] + part_d[(uint64_t)f * nblocks + b];
#pragma unroll
        for (int f = 0; f < (int)MET_K_FIELDS; f++) {
            const uint64_t v = part_k[(uint64_t)f * nblocks + b];
            k[f] = v > k[f] ? v : k[f];
        }
#pragma unroll
        for (int f = 0; f < (int)MET_U_FIELDS; f++) c[f] += part_u[(uint64_t)f * nblocks + b];
    }
#pragma unroll
    for (int f = 0; f < (int)MET_D_FIELDS; f++) d[f] = metrics_wave_add_f64(d[f]);
#pragma unroll
    for (int f = 0; f < (int)MET_K_FIELDS; f++) k[f] = wave_reduce_max64(k[f]);
#pragma unroll
    for (int f = 0; f < (int)MET_U_FIELDS; f++) c[f] = wave_reduce_add64(c[f]);
    if (lane == 0u) {
#pragma unroll
        for (int f = 0; f < (int)MET_D_FIELDS; f++) s_d[wid][f] = d[f];
#pragma unroll
        for (int f = 0; f < (int)MET_K_FIELDS; f++) s_k[wid][f] = k[f];
#pragma unroll
        for (int f = 0; f < (int)MET_U_FIELDS; f++) s_c[wid][f] = c[f];
    }
    __syncthreads();
    const uint32_t f = threadIdx.x;
    if (f < MET_D_FIELDS) {
        const double v = (s_d[0][f] + s_d[1][f]) + (s_d[2][f] + s_d[3][f]);
        if (f < 4u) out->sum_sq[f] = v;
        else if (f < 8u) out->sum_abs[f - 4u] = v;
        else out->ssim_sum[f - 8u] = v;
    } else if (f >= 64u && f < 64u + MET_K_FIELDS) {
        const uint32_t g = f - 64u;
        const uint64_t m01 = s_k[0][g] > s_k[1][g] ? s_k[0][g] : s_k[1][g], m23 = s_k[2][g] > s_k[3][g] ? s_k[2][g] : s_k[3][g];
        const uint64_t v = m01 > m23 ? m01 : m23;
        out->max_abs[g] = u2f((uint32_t)(v >> 32));
        out->max_abs_at[g] = ~(uint32_t)v;
    } else if (f >= 128u && f < 128u + MET_U_FIELDS) {
        const uint32_t g = f - 128u;
        const uint64_t v = (s_c[0][g] + s_c[1][g]) + (s_c[2][g] + s_c[3][g]);
        if (g == 0u) out->finite = v;
        else if (g == 1u) out->differing = v;
        else if (g == 2u) out->bit_differing = v;
        else out->ssim_finite[g - 3u] = v;
    } else if (f == 192u) {
        out->pixels = pixels;
    }
}

}  // namespace gs
