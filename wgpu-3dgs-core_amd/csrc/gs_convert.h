// gs_convert.h — source-format record -> struct Gaussian conversions as ONE set of host + device
// functions: Gaussian::from_ply (src/gaussian.rs:70-92).  The host entry point
// (gs_gaussian_from_ply, gs_ply.cpp) and the device kernel (k_from_ply_pods, gs_pack_kernels.h) both call
// ply_to_gaussian_words below, so a scene loaded on the device is bit-identical to one converted on
// the host by construction.
//
// exp: the reference calls f32::exp, which on Linux is glibc's expf.  A device `expf` (ocml) is a
// different algorithm and differs from it in the last bit, so BOTH sides use gs_expf below: the
// published algorithm glibc (>= 2.27), musl, newlib and bionic share — Szabolcs Nagy's expf from
// ARM optimized-routines (math/expf.c, math/exp2f_data.c; EXP2F_TABLE_BITS = 5): the argument is
// reduced in DOUBLE to k/32 + r, 2^(k/32) comes from a 32-entry table, a cubic in r finishes, and the
// double result is rounded to binary32 once (worst-case error 0.502 ulp).  Every operation is an IEEE
// double +, *, or a conversion, written without contraction, so host and device agree bit for bit,
// and both agree with libm wherever the double result is not within ~1e-9 ulp of a binary32 rounding
// boundary (tests/test_ply.py: 0 differences in 4 M samples; reference tolerance 1e-4,
// tests/common/assert.rs:4).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIP__) || defined(__HIPCC_RTC__)
#define GS_HD __host__ __device__
#else
#define GS_HD
#endif
// loops whose indices must be constants where the arrays are a kernel's registers
#if defined(__clang__)
#define GS_UNROLL _Pragma("unroll")
#else
#define GS_UNROLL
#endif

namespace gs {

GS_HD inline uint32_t cv_f2u(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
GS_HD inline float cv_u2f(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
GS_HD inline uint64_t cv_d2u(double d) {
    uint64_t u;
    memcpy(&u, &d, 8);
    return u;
}
GS_HD inline double cv_u2d(uint64_t u) {
    double d;
    memcpy(&d, &u, 8);
    return d;
}

// IEEE 754 leaves the sign and payload of a NaN that ARITHMETIC produces to the implementation: x86
// returns the negative quiet NaN (0xffc00000) for 0/0 and propagates operand payloads, gfx950 returns
// +qNaN (0x7fc00000).  Values computed from degenerate input (a zero or infinite quaternion) are
// therefore canonicalised to +qNaN wherever host and device must agree bit for bit.
GS_HD inline uint32_t cv_canon_nan_bits(float f) { return f != f ? 0x7fc00000u : cv_f2u(f); }

// T[i] = bits(2^(i/32)) - (i << 47), 2^(i/32) correctly rounded to binary64
GS_HD inline uint64_t expf_table(uint32_t i) {
    const uint64_t T[32] = {
        0x3ff0000000000000ull, 0x3fefd9b0d3158574ull, 0x3fefb5586cf9890full, 0x3fef9301d0125b51ull,
        0x3fef72b83c7d517bull, 0x3fef54873168b9aaull, 0x3fef387a6e756238ull, 0x3fef1e9df51fdee1ull,
        0x3fef06fe0a31b715ull, 0x3feef1a7373aa9cbull, 0x3feedea64c123422ull, 0x3feece086061892dull,
        0x3feebfdad5362a27ull, 0x3feeb42b569d4f82ull, 0x3feeab07dd485429ull, 0x3feea47eb03a5585ull,
        0x3feea09e667f3bcdull, 0x3fee9f75e8ec5f74ull, 0x3feea11473eb0187ull, 0x3feea589994cce13ull,
        0x3feeace5422aa0dbull, 0x3feeb737b0cdc5e5ull, 0x3feec49182a3f090ull, 0x3feed503b23e255dull,
        0x3feee89f995ad3adull, 0x3feeff76f2fb5e47ull, 0x3fef199bdd85529cull, 0x3fef3720dcef9069ull,
        0x3fef5818dcfba487ull, 0x3fef7c97337b9b5full, 0x3fefa4afa2a490daull, 0x3fefd0765b6e4540ull};
    return T[i & 31u];
}

// expf for every binary32 input (NaN -> NaN, +inf -> +inf, -inf -> 0, overflow -> +inf,
// underflow -> 0 / subnormals rounded once)
GS_HD inline float gs_expf(float x) {
    const uint32_t ux = cv_f2u(x);
    const uint32_t abstop = (ux >> 20) & 0x7ffu;
    if (abstop >= 0x42bu) {                         // |x| >= 88 or NaN / inf
        if (ux == 0xff800000u) return 0.0f;         // -inf
        if (abstop >= 0x7f8u) return x + x;         // NaN, +inf
        if (x > 88.72283172607421875f) return cv_u2f(0x7f800000u);   // x > log(2^128)
        if (x < -103.972076416015625f) return 0.0f;                  // x < log(2^-150)
    }
    const double N = 32.0;
    const double inv_ln2_n = 0x1.71547652b82fep+0 * N;
    const double shift = 0x1.8p+52;
    const double c0 = 0x1.c6af84b912394p-5 / N / N / N, c1 = 0x1.ebfce50fac4f3p-3 / N / N, c2 = 0x1.62e42ff0c52d6p-1 / N;
    const double z = inv_ln2_n * (double)x;
    double kd = z + shift;                          // round to nearest integer in the low bits
    const uint64_t ki = cv_d2u(kd);
    kd = kd - shift;
    const double r = z - kd;
    const uint64_t t = expf_table((uint32_t)ki) + (ki << 47);
    const double s = cv_u2d(t);
    const double p = c0 * r + c1;
    const double r2 = r * r;
    double y = c2 * r + 1.0;
    y = p * r2 + y;
    y = y * s;
    return (float)y;
}

// log: the reference calls f32::ln (gaussian.rs:100,105,254), glibc's logf — Szabolcs Nagy's logf from ARM
// optimized-routines (math/logf.c, math/logf_data.c; LOGF_TABLE_BITS = 4): x = 2^k z with z in [0x1.66p-1, 0x1.66p0),
// c = the centre of z's sixteenth of that interval, log x = log(z / c) + log c + k ln 2 with a cubic in r = z / c - 1,
// evaluated in DOUBLE and rounded to binary32 once.  As gs_expf: IEEE double +, * and conversions only, written without
// contraction, so host and device agree bit for bit.
GS_HD inline double logf_invc(uint32_t i) {
    const double T[16] = {0x1.661ec79f8f3bep+0, 0x1.571ed4aaf883dp+0, 0x1.49539f0f010bp+0,  0x1.3c995b0b80385p+0,
                          0x1.30d190c8864a5p+0, 0x1.25e227b0b8eap+0,  0x1.1bb4a4a1a343fp+0, 0x1.12358f08ae5bap+0,
                          0x1.0953f419900a7p+0, 0x1p+0,               0x1.e608cfd9a47acp-1, 0x1.ca4b31f026aap-1,
                          0x1.b2036576afce6p-1, 0x1.9c2d163a1aa2dp-1, 0x1.886e6037841edp-1, 0x1.767dcf5534862p-1};
    return T[i & 15u];
}
GS_HD inline double logf_logc(uint32_t i) {
    const double T[16] = {-0x1.57bf7808caadep-2, -0x1.2bef0a7c06ddbp-2, -0x1.01eae7f513a67p-2, -0x1.b31d8a68224e9p-3,
                          -0x1.6574f0ac07758p-3, -0x1.1aa2bc79c81p-3,   -0x1.a4e76ce8c0e5ep-4, -0x1.1973c5a611cccp-4,
                          -0x1.252f438e10c1ep-5, 0.0,                   0x1.aa5aa5df25984p-5,  0x1.c5e53aa362eb4p-4,
                          0x1.526e57720db08p-3,  0x1.bc2860d22477p-3,   0x1.1058bc8a07ee1p-2,  0x1.4043057b6ee09p-2};
    return T[i & 15u];
}

// logf for every binary32 input: +-0 -> -inf, +inf -> +inf, NaN -> the NaN quieted, negative (and -inf) -> the default
// NaN x86 produces for 0/0 (0xffc00000: what glibc's (x - x) / (x - x) returns there), subnormals through the normal path
GS_HD inline float gs_logf(float x) {
    uint32_t ix = cv_f2u(x);
    if (ix == 0x3f800000u) return 0.0f;
    if (ix - 0x00800000u >= 0x7f000000u) {             // zero, subnormal, negative, inf, NaN
        if ((ix << 1) == 0u) return cv_u2f(0xff800000u);
        if (ix == 0x7f800000u) return x;
        if ((ix << 1) > 0xff000000u) return cv_u2f(ix | 0x00400000u);
        if (ix & 0x80000000u) return cv_u2f(0xffc00000u);
        // bits(x * 2^23) - (23 << 23): x = ix * 2^-149 and the conversion of ix < 2^23 is exact, so this is an integer
        // identity and does not depend on how the device treats a subnormal operand
        ix = cv_f2u((float)ix) - (149u << 23);
    }
    const uint32_t tmp = ix - 0x3f330000u;
    const uint32_t i = (tmp >> 19) & 15u;
    const int32_t k = (int32_t)tmp >> 23;
    const uint32_t iz = ix - (tmp & 0xff800000u);
    const double z = (double)cv_u2f(iz);
    const double ln2 = 0x1.62e42fefa39efp-1;
    const double a0 = -0x1.00ea348b88334p-2, a1 = 0x1.5575b0be00b6ap-2, a2 = -0x1.ffffef20a4123p-2;
    const double r = z * logf_invc(i) - 1.0;
    const double y0 = logf_logc(i) + (double)k * ln2;
    const double r2 = r * r;
    double y = a1 * r + a2;
    y = a0 * r2 + y;
    y = y * r2 + (y0 + r);
    return (float)y;
}

// Rust `as u8` of an f32: truncating, saturating, NaN -> 0
GS_HD inline uint32_t cv_sat_u8(float v) {
    if (!(v > 0.0f)) return 0u;
    if (v >= 255.0f) return 255u;
    return (uint32_t)(int)v;
}
GS_HD inline float cv_clamp_0_255(float v) {       // glam Vec4::clamp = max(lo).min(hi): NaN -> lo (sat_u8 maps it to 0 anyway)
    float a = v > 0.0f ? v : 0.0f;
    if (v != v) a = 0.0f;
    return a < 255.0f ? a : 255.0f;
}

// struct Gaussian word offsets (include/gs3d.h gs_gaussian): rot xyzw @0, pos @4, color u8x4 @7,
// sh[45] @8, scale @53; PlyGaussianPod (62 f32): pos @0, normal @3, f_dc @6, f_rest @9, opacity @54,
// scale @55, rot wxyz @58
constexpr int PLY_WORDS = 62;
constexpr int CV_GAUSSIAN_WORDS = 56;

// Gaussian::from_ply (src/gaussian.rs:70-92): p = 62 words of one PlyGaussianPod, g = 56 words out.
// `sqrtf_cr` must be a correctly rounded binary32 square root (host sqrtf; device sqrtf, which hipcc rounds correctly by default — NOT __fsqrt_rn, the native approximation).
template <class Sqrt>
GS_HD inline void ply_to_gaussian_words(const uint32_t *p, uint32_t *g, Sqrt sqrtf_cr) {
    g[4] = p[0];
    g[5] = p[1];
    g[6] = p[2];
    // Quat::from_xyzw(rot[1], rot[2], rot[3], rot[0]).normalize()
    const float q[4] = {cv_u2f(p[59]), cv_u2f(p[60]), cv_u2f(p[61]), cv_u2f(p[58])};
    const float len = sqrtf_cr(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    for (int k = 0; k < 4; k++) g[k] = cv_canon_nan_bits(q[k] / len);
    for (int k = 0; k < 3; k++) g[53 + k] = cv_canon_nan_bits(gs_expf(cv_u2f(p[55 + k])));
    uint32_t color = 0;
    for (int k = 0; k < 3; k++) {
        const float v = (cv_u2f(p[6 + k]) * 0.2820948f + 0.5f) * 255.0f;        // SH0_TO_LINEAR_FACTOR
        color |= cv_sat_u8(cv_clamp_0_255(v)) << (8 * k);
    }
    const float a = (1.0f / (1.0f + gs_expf(-cv_u2f(p[54])))) * 255.0f;
    color |= cv_sat_u8(cv_clamp_0_255(a)) << 24;
    g[7] = color;
    for (int k = 0; k < 15; k++) {       // channel-planar f_rest -> RGB-interleaved
        g[8 + 3 * k + 0] = p[9 + k];
        g[8 + 3 * k + 1] = p[9 + k + 15];
        g[8 + 3 * k + 2] = p[9 + k + 30];
    }
}

// ---- covariance -> rotation + scale (no reference item) ----

// One Jacobi rotation of the pair (p, q); r is the third index.  app / aqq / apq: the pair's terms, arp / arq: the other two
// off-diagonals, (v0p, v0q) .. (v2p, v2q): columns p and q of V.  Skipped exactly when apq == 0: the arithmetic runs anyway
// (a kernel predicates; what 0 / 0 gives is discarded) and the selects keep the old values bit for bit.  3 divisions and 2
// square roots, every operation a rounded binary32 one.
template <class Sqrt>
GS_HD inline void cov3d_jacobi_rotate(float &app, float &aqq, float &apq, float &arp, float &arq, float &v0p, float &v0q, float &v1p,
                                      float &v1q, float &v2p, float &v2q, Sqrt sqrtf_cr) {
    const bool on = apq != 0.0f;
    const float theta = (aqq - app) / (2.0f * apq);
    const float t = (theta < 0.0f ? -1.0f : 1.0f) / (cv_u2f(cv_f2u(theta) & 0x7fffffffu) + sqrtf_cr(theta * theta + 1.0f));
    const float c = 1.0f / sqrtf_cr(t * t + 1.0f);
    const float s = t * c;
    const float tapq = t * apq;
    const float npp = app - tapq, nqq = aqq + tapq;
    const float nrp = c * arp - s * arq, nrq = s * arp + c * arq;
    const float n0p = c * v0p - s * v0q, n0q = s * v0p + c * v0q;
    const float n1p = c * v1p - s * v1q, n1q = s * v1p + c * v1q;
    const float n2p = c * v2p - s * v2q, n2q = s * v2p + c * v2q;
    app = on ? npp : app;
    aqq = on ? nqq : aqq;
    apq = on ? 0.0f : apq;
    arp = on ? nrp : arp;
    arq = on ? nrq : arq;
    v0p = on ? n0p : v0p;
    v0q = on ? n0q : v0q;
    v1p = on ? n1p : v1p;
    v1q = on ? n1q : v1q;
    v2p = on ? n2p : v2p;
    v2q = on ? n2q : v2q;
}

constexpr int COV3D_JACOBI_SWEEPS = 6;      // fixed (NOTES.md: 5 and 6 sweeps give the same bits on 200 000 covariances)

// decompose: c = the six covariance terms xx, yx, zx, yy, zy, zz as cov3d_from_rot_scale writes them ->
// q = unit quaternion xyzw with w >= 0, s = the three scales in Jacobi's own column order: (R S)(R S)^T = C up to rounding,
// negative eigenvalues clamped to 0.  Every operation is a rounded binary32 +, -, *, / or square root in the order written
// (no contraction), so host and device give the same bits.  `sqrtf_cr`: a correctly rounded binary32 square root, as above.
template <class Sqrt>
GS_HD inline void cov3d_decompose(const float c[6], float q[4], float s[3], Sqrt sqrtf_cr) {
    // 1, 2: non-finite and zero input, from the bits; m = the largest |c_k| (as bits: the order of the magnitudes)
    uint32_t m = 0u;
    GS_UNROLL
    for (int k = 0; k < 6; k++) {
        const uint32_t a = cv_f2u(c[k]) & 0x7fffffffu;
        m = a > m ? a : m;
    }
    q[0] = 0.0f;
    q[1] = 0.0f;
    q[2] = 0.0f;
    q[3] = 1.0f;
    if (m >= 0x7f800000u || m == 0u) {
        s[0] = s[1] = s[2] = cv_u2f(m ? 0x7fc00000u : 0u);
        return;
    }
    // 3: prescale by 2^-e, e even, so that the largest word lands in [1, 4).  A subnormal maximum is first lifted by 2^24
    // (exact, even), which makes its exponent field >= 2.  Both factors are built from their exponent bits.
    const uint32_t lift = m < 0x00800000u ? 24u : 0u;
    const float pre = cv_u2f((127u + lift) << 23);                                      // 2^lift
    const uint32_t mexp = cv_f2u(cv_u2f(m) * pre) >> 23;                                // biased exponent of the maximum, 1..254
    const int32_t e = (int32_t)((mexp + 1u) & ~1u) - 128;                               // mexp - 127 rounded down to even, -126..126
    const float down = cv_u2f((uint32_t)(127 - e) << 23);                               // 2^-e
    const float up = cv_u2f((uint32_t)(127 + (e - (int32_t)lift) / 2) << 23);           // 2^((e - lift) / 2)
    float a00 = c[0] * pre * down, a01 = c[1] * pre * down, a02 = c[2] * pre * down;
    float a11 = c[3] * pre * down, a12 = c[4] * pre * down, a22 = c[5] * pre * down;
    // 4: cyclic Jacobi, pairs (0,1), (0,2), (1,2), a fixed number of sweeps; v<row><column>
    float v00 = 1.0f, v01 = 0.0f, v02 = 0.0f, v10 = 0.0f, v11 = 1.0f, v12 = 0.0f, v20 = 0.0f, v21 = 0.0f, v22 = 1.0f;
    for (int sweep = 0; sweep < COV3D_JACOBI_SWEEPS; sweep++) {
        cov3d_jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21, sqrtf_cr);      // (0,1), r = 2
        cov3d_jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22, sqrtf_cr);      // (0,2), r = 1
        cov3d_jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22, sqrtf_cr);      // (1,2), r = 0
    }
    // 5: scales, unsorted; a negative eigenvalue (and -0) gives +0
    s[0] = sqrtf_cr(a00 > 0.0f ? a00 : 0.0f) * up;
    s[1] = sqrtf_cr(a11 > 0.0f ? a11 : 0.0f) * up;
    s[2] = sqrtf_cr(a22 > 0.0f ? a22 : 0.0f) * up;
    // 6: V -> quaternion with the branches of glam's Quat::from_mat3 (m<column><row> = v<row><column>), normalised as
    // ply_to_gaussian_words normalises, w >= 0
    float x, y, z, w;
    if (v22 <= 0.0f) {
        const float dif10 = v11 - v00, omm22 = 1.0f - v22;
        if (dif10 <= 0.0f) {
            const float four = omm22 - dif10, inv = 0.5f / sqrtf_cr(four);
            x = four * inv, y = (v10 + v01) * inv, z = (v20 + v02) * inv, w = (v21 - v12) * inv;
        } else {
            const float four = omm22 + dif10, inv = 0.5f / sqrtf_cr(four);
            x = (v10 + v01) * inv, y = four * inv, z = (v21 + v12) * inv, w = (v02 - v20) * inv;
        }
    } else {
        const float sum10 = v11 + v00, opm22 = 1.0f + v22;
        if (sum10 <= 0.0f) {
            const float four = opm22 - sum10, inv = 0.5f / sqrtf_cr(four);
            x = (v20 + v02) * inv, y = (v21 + v12) * inv, z = four * inv, w = (v10 - v01) * inv;
        } else {
            const float four = opm22 + sum10, inv = 0.5f / sqrtf_cr(four);
            x = (v21 - v12) * inv, y = (v02 - v20) * inv, z = (v10 - v01) * inv, w = four * inv;
        }
    }
    const float len = sqrtf_cr(((x * x + y * y) + z * z) + w * w);
    const bool neg = w < 0.0f;
    q[0] = neg ? -(x / len) : x / len;
    q[1] = neg ? -(y / len) : y / len;
    q[2] = neg ? -(z / len) : z / len;
    q[3] = neg ? -(w / len) : w / len;
}

// ---- Gaussian::from_spz (src/gaussian.rs:134-229) over the decompressed columns (spz.rs:739-771) ----

// where the columns of a decompressed SPZ payload start (positions -> alphas -> colors -> scales ->
// rotations -> sh) and how to read them; pointers may be host or device memory
struct SpzView {
    const uint8_t *pos, *alpha, *color, *scale, *rot, *sh;
    uint32_t version;           // 1..3: f16 vs 24-bit fixed positions; first-three vs smallest-three quaternions
    uint32_t fractional_bits;
    uint32_t ncoef;             // SH coefficients per channel: 0, 3, 8, 15
};

GS_HD inline float cv_f16_to_f32(uint32_t h) {
    const uint32_t sign = (h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
    if (e == 0) return cv_u2f(cv_f2u((float)m * 5.9604644775390625e-08f) | sign);      // m * 2^-24, exact
    if (e == 31) return cv_u2f(sign | 0x7f800000u | (m << 13));
    return cv_u2f(sign | ((e + 112u) << 23) | (m << 13));
}

// SPZ_COLOR_TO_LINEAR_FRAC_A_B = 0.2820948 / 0.15, SPZ_COLOR_TO_LINEAR_C = (1 - A_B) * (0.5 * 255) — gaussian.rs:127-131
GS_HD inline float spz_color_ab() { return 0.2820948f / 0.15f; }
GS_HD inline float spz_color_c() { return (1.0f - spz_color_ab()) * (0.5f * 255.0f); }

template <class Sqrt>
GS_HD inline void spz_to_gaussian_words(const SpzView &v, size_t i, uint32_t *g, Sqrt sqrtf_cr) {
    if (v.version == 1) {
        for (int c = 0; c < 3; c++) {
            const uint8_t *p = v.pos + 6 * i + 2 * c;
            g[4 + c] = cv_f2u(cv_f16_to_f32((uint32_t)p[0] | ((uint32_t)p[1] << 8)));
        }
    } else {
        // `1 << fractional_bits` on i32 as Rust evaluates it in release builds (shift count masked to 5
        // bits); the header byte is untrusted, so the plain C shift would be undefined behaviour
        const float s = 1.0f / (float)(int32_t)(1u << (v.fractional_bits & 31u));
        for (int c = 0; c < 3; c++) {
            const uint8_t *p = v.pos + 9 * i + 3 * c;
            int32_t fixed = (int32_t)p[0] | ((int32_t)p[1] << 8) | ((int32_t)p[2] << 16);
            if (fixed & 0x800000) fixed |= (int32_t)0xff000000u;
            g[4 + c] = cv_f2u((float)fixed * s);
        }
    }
    for (int c = 0; c < 3; c++) g[53 + c] = cv_f2u(gs_expf((float)v.scale[3 * i + c] / 16.0f - 10.0f));
    if (v.version < 3) {
        const float x = (float)v.rot[3 * i] / 127.5f - 1.0f, y = (float)v.rot[3 * i + 1] / 127.5f - 1.0f,
                    z = (float)v.rot[3 * i + 2] / 127.5f - 1.0f;
        const float l2 = (x * x + y * y) + z * z;
        const float w2 = 1.0f - l2;
        g[0] = cv_f2u(x);
        g[1] = cv_f2u(y);
        g[2] = cv_f2u(z);
        g[3] = cv_f2u(sqrtf_cr(w2 > 0.0f ? w2 : 0.0f));        // f32::max(.., 0.0): NaN -> 0
    } else {
        const uint8_t *q = v.rot + 4 * i;
        uint32_t comp = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
        const uint32_t mask = (1u << 9) - 1u;
        const uint32_t largest = comp >> 30;
        float sum = 0.0f, comps[4];
        for (uint32_t k = 0; k < 4; k++) {   // ascending, as the reference's array::from_fn
            if (k == largest) {
                comps[k] = 0.0f;
                continue;
            }
            const uint32_t mag = comp & mask, neg = (comp >> 9) & 1u;
            comp >>= 10;
            const float val = 0.70710678118654752440f * ((float)mag / (float)mask) * (neg ? -1.0f : 1.0f);
            sum += val * val;
            comps[k] = val;
        }
        const float w2 = 1.0f - sum;
        for (uint32_t k = 0; k < 4; k++) g[k] = cv_f2u(k == largest ? sqrtf_cr(w2 > 0.0f ? w2 : 0.0f) : comps[k]);
    }
    uint32_t color = 0;
    for (int c = 0; c < 3; c++) {
        const float val = (float)v.color[3 * i + c] * spz_color_ab() + spz_color_c();
        color |= cv_sat_u8(cv_clamp_0_255(val)) << (8 * c);
    }
    color |= (uint32_t)v.alpha[i] << 24;
    g[7] = color;
    for (int k = 0; k < 45; k++) g[8 + k] = 0u;
    for (uint32_t k = 0; k < v.ncoef; k++)
        for (int c = 0; c < 3; c++) g[8 + 3 * k + c] = cv_f2u(((float)v.sh[(i * v.ncoef + k) * 3 + c] - 128.0f) / 128.0f);
}

// ---- struct Gaussian -> source-format records: Gaussian::to_ply (gaussian.rs:95-125) and Gaussian::to_spz
// (gaussian.rs:227-352), shared by the host entry points (gs_gaussian_to_ply, gs_spz_encode_decompressed) and the export
// kernels (gs_export_kernels.h).  min / max / clamp are written as comparisons (NaN -> the lower bound, as f32::max(lo)
// .min(hi) gives) and every value that reaches the output goes through gs_logf, a correctly rounded IEEE operation or an
// integer: host and device produce the same bytes.

// g = 56 words of one struct Gaussian, p = 62 words of one PlyGaussianPod out
GS_HD inline void gaussian_to_ply_words(const uint32_t *g, uint32_t *p) {
    p[0] = g[4];
    p[1] = g[5];
    p[2] = g[6];
    p[3] = 0u;                       // normal (0, 0, 1)
    p[4] = 0u;
    p[5] = 0x3f800000u;
    const uint32_t color = g[7];
    GS_UNROLL
    for (int k = 0; k < 3; k++) {
        const float c = (float)((color >> (8 * k)) & 0xffu) / 255.0f;
        p[6 + k] = cv_f2u((c - 0.5f) / 0.2820948f);
    }
    GS_UNROLL
    for (int k = 0; k < 15; k++) {       // RGB-interleaved -> channel-planar f_rest
        p[9 + k] = g[8 + 3 * k + 0];
        p[9 + k + 15] = g[8 + 3 * k + 1];
        p[9 + k + 30] = g[8 + 3 * k + 2];
    }
    const float a = (float)(color >> 24) / 255.0f;
    p[54] = cv_f2u(-gs_logf(1.0f / a - 1.0f));      // the argument is >= 0 or +inf: never a NaN whose sign the negation would flip
    GS_UNROLL
    for (int k = 0; k < 3; k++) p[55 + k] = cv_f2u(gs_logf(cv_u2f(g[53 + k])));
    p[58] = g[3];                    // rot wxyz
    p[59] = g[0];
    p[60] = g[1];
    p[61] = g[2];
}

// half 2.x f16::from_f32 (const conversion == IEEE RNE; every NaN becomes 0x7e00 | sign)
GS_HD inline uint32_t cv_f32_to_f16(float value) {
    const uint32_t f32infty = 255u << 23, f16max = (127u + 16u) << 23;
    const uint32_t magic = ((127u - 15u) + (23u - 10u) + 1u) << 23;
    uint32_t u = cv_f2u(value);
    const uint32_t sign = u & 0x80000000u;
    u ^= sign;
    uint32_t o;
    if (u >= f16max) {
        o = u > f32infty ? 0x7e00u : 0x7c00u;
    } else if (u < (113u << 23)) {
        o = cv_f2u(cv_u2f(u) + cv_u2f(magic)) - magic;
    } else {
        const uint32_t odd = (u >> 13) & 1u;
        u += ((uint32_t)(15 - 127) << 23) + 0xfffu;
        u += odd;
        o = u >> 13;
    }
    return (o & 0xffffu) | (sign >> 16);
}
// Rust `as u32` / `as i32` of an f32: truncating, saturating, NaN -> 0
GS_HD inline uint32_t cv_sat_u32(float v) { return !(v > 0.0f) ? 0u : v >= 4294967295.0f ? 0xffffffffu : (uint32_t)v; }
GS_HD inline int32_t cv_sat_i32(float v) {
    return v != v ? 0 : v >= 2147483647.0f ? 2147483647 : v <= -2147483648.0f ? (int32_t)0x80000000u : (int32_t)v;
}
// f32::max(lo).min(hi) for lo <= hi: NaN -> lo
GS_HD inline float cv_clamp(float v, float lo, float hi) {
    const float a = v > lo ? v : lo;
    return a < hi ? a : hi;
}
GS_HD inline float cv_fabs(float v) { return cv_u2f(cv_f2u(v) & 0x7fffffffu); }
// gaussian.rs:317-324: only buckets when bucket < 8
GS_HD inline uint32_t spz_quantize_sh(float x, uint32_t bucket) {
    uint32_t q = cv_sat_u32(roundf(x * 128.0f + 128.0f));
    if (!(bucket >= 8u)) q = (q + bucket / 2u) / bucket * bucket;
    return q > 255u ? 255u : q;
}

// the six columns of a decompressed SPZ payload, in file order, and their bytes per record
enum { SPZ_COL_POS = 0, SPZ_COL_ALPHA = 1, SPZ_COL_COLOR = 2, SPZ_COL_SCALE = 3, SPZ_COL_ROT = 4, SPZ_COL_SH = 5 };
GS_HD inline uint32_t spz_col_bytes(int col, uint32_t version, uint32_t ncoef) {
    return col == SPZ_COL_POS ? (version == 1u ? 6u : 9u) : col == SPZ_COL_ALPHA ? 1u : col == SPZ_COL_ROT ? (version >= 3u ? 4u : 3u)
           : col == SPZ_COL_SH ? 3u * ncoef : 3u;
}

// g = 56 words of one struct Gaussian; put(column, k, byte) receives byte k of the record's entry in each column.
// bucket = 1 << (8 - quantize bits of the degree).  `sqrtf_cr`: a correctly rounded binary32 square root, as above.
template <class Put, class Sqrt>
GS_HD inline void gaussian_to_spz_bytes(const uint32_t *g, uint32_t version, uint32_t fractional_bits, uint32_t ncoef, uint32_t bucket,
                                        Put put, Sqrt sqrtf_cr) {
    if (version == 1u) {
        GS_UNROLL
        for (int c = 0; c < 3; c++) {
            const uint32_t h = cv_f32_to_f16(cv_u2f(g[4 + c]));
            put(SPZ_COL_POS, 2 * c, h & 0xffu);
            put(SPZ_COL_POS, 2 * c + 1, h >> 8);
        }
    } else {
        const float s = (float)(int32_t)(1u << (fractional_bits & 31u));
        GS_UNROLL
        for (int c = 0; c < 3; c++) {
            const uint32_t fixed = (uint32_t)cv_sat_i32(roundf(cv_u2f(g[4 + c]) * s));
            put(SPZ_COL_POS, 3 * c, fixed & 0xffu);
            put(SPZ_COL_POS, 3 * c + 1, (fixed >> 8) & 0xffu);
            put(SPZ_COL_POS, 3 * c + 2, (fixed >> 16) & 0xffu);
        }
    }
    GS_UNROLL
    for (int c = 0; c < 3; c++) {
        const float v = roundf((gs_logf(cv_u2f(g[53 + c])) + 10.0f) * 16.0f);
        put(SPZ_COL_SCALE, c, cv_sat_u8(cv_clamp(v, 0.0f, 255.0f)));
    }
    // Quat::normalize
    float q[4];
    {
        const float r0 = cv_u2f(g[0]), r1 = cv_u2f(g[1]), r2 = cv_u2f(g[2]), r3 = cv_u2f(g[3]);
        const float len = sqrtf_cr(((r0 * r0 + r1 * r1) + r2 * r2) + r3 * r3);
        q[0] = r0 / len;
        q[1] = r1 / len;
        q[2] = r2 / len;
        q[3] = r3 / len;
    }
    if (version >= 3u) {
        uint32_t largest = 0;
        GS_UNROLL
        for (uint32_t k = 1; k < 4; k++) {       // max_by keeps the LAST maximum
            float cur = cv_fabs(q[0]);
            GS_UNROLL
            for (uint32_t j = 1; j < 4; j++)
                if (j == largest) cur = cv_fabs(q[j]);
            if (!(cv_fabs(q[k]) < cur)) largest = k;     // ... and a NaN compares Equal (partial_cmp(..).unwrap_or(Equal))
        }
        const uint32_t mask = (1u << 9) - 1u;
        float ql = q[0];
        GS_UNROLL
        for (uint32_t j = 1; j < 4; j++)
            if (j == largest) ql = q[j];
        const uint32_t negate = ql < 0.0f ? 1u : 0u;
        uint32_t comp = largest;
        GS_UNROLL
        for (uint32_t k = 0; k < 4; k++) {
            if (k == largest) continue;
            const uint32_t neg = (q[k] < 0.0f ? 1u : 0u) ^ negate;
            const float mv = (float)mask * (cv_fabs(q[k]) * 1.41421356237309504880f) + 0.5f;
            const uint32_t mag = cv_sat_u32(cv_clamp(mv, 0.0f, (float)mask - 1.0f));
            comp = (comp << 10) | (neg << 9) | mag;
        }
        GS_UNROLL
        for (int b = 0; b < 4; b++) put(SPZ_COL_ROT, b, (comp >> (8 * b)) & 0xffu);
    } else {
        const bool flip = q[3] < 0.0f;
        GS_UNROLL
        for (int c = 0; c < 3; c++) {
            const float v = roundf(((flip ? -q[c] : q[c]) + 1.0f) * 127.5f);
            put(SPZ_COL_ROT, c, cv_sat_u8(cv_clamp(v, 0.0f, 255.0f)));
        }
    }
    const uint32_t color = g[7];
    put(SPZ_COL_ALPHA, 0, color >> 24);
    GS_UNROLL
    for (int c = 0; c < 3; c++) {
        const float v = ((float)((color >> (8 * c)) & 0xffu) - spz_color_c()) / spz_color_ab();
        put(SPZ_COL_COLOR, c, cv_sat_u8(cv_clamp(v, 0.0f, 255.0f)));
    }
    GS_UNROLL
    for (uint32_t k = 0; k < 15u; k++)
        if (k < ncoef)
            GS_UNROLL
            for (int c = 0; c < 3; c++) put(SPZ_COL_SH, (int)(3u * k) + c, spz_quantize_sh(cv_u2f(g[8 + 3 * k + c]), bucket));
}

}  // namespace gs
