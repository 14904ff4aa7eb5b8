// gs_relayout.hip — conversion of records between the 12 POD layouts: the pair table, the host
// conversion, the converted extraction and the concatenation of sources of any layouts (§3.9's, with a target layout); the
// decomposition of covariance layouts into rotation + scale (§3.12a), on the host and fused with the extraction.
// Kernels: gs_relayout_kernels.h; the extraction scan and the plain copy are gs_edit.hip's.
#include "gs_host.h"

#include "gs_relayout_kernels.h"

using namespace gsh;

extern "C" int32_t gs_layout_convertible(gs_sh_config src_sh, gs_cov3d_config src_cov, gs_sh_config dst_sh, gs_cov3d_config dst_cov) {
    return gs::layout_convertible((int)src_sh, (int)src_cov, (int)dst_sh, (int)dst_cov) ? 1 : 0;
}

// the checks every conversion entry shares: both layouts known, the pair defined
static gs_status check_pair(int ssh, int scov, int dsh, int dcov) {
    if (!valid_cfg(ssh, scov) || !valid_cfg(dsh, dcov)) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "unknown layout config");
    if (!gs::layout_convertible(ssh, scov, dsh, dcov))
        return gs_fail(GS_ERR_LOSSY_CONFIG, (uint64_t)scov, (uint64_t)dcov, 0, "Cannot convert a covariance back to rotation and scale");
    return GS_OK;
}

extern "C" gs_status gs_convert_pods(gs_sh_config src_sh, gs_cov3d_config src_cov, gs_sh_config dst_sh, gs_cov3d_config dst_cov,
                                     const void *pods, size_t n, void *out) {
    if (!pods || !out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    GS_TRY(check_pair(src_sh, src_cov, dst_sh, dst_cov));
    const size_t ss = (size_t)gs::pod_bytes(src_sh, src_cov), ds = (size_t)gs::pod_bytes(dst_sh, dst_cov);
    const uint8_t *in = (const uint8_t *)pods;
    uint8_t *o = (uint8_t *)out;
    if (src_sh == dst_sh && src_cov == dst_cov) {      // identical layouts keep every byte, the trailing pad too
        std::memcpy(o, in, n * ss);
        return GS_OK;
    }
    for (size_t i = 0; i < n; i++) {
        uint32_t pw[56], ow[56];
        std::memcpy(pw, in + i * ss, ss);
        gs::convert_words(src_sh, src_cov, dst_sh, dst_cov, pw, ow);      // the same code the device kernel runs
        std::memcpy(o + i * ds, ow, ds);
    }
    return GS_OK;
}

extern "C" void gs_cov3d_decompose(const float cov[6], float rot_xyzw[4], float scale[3]) {
    gs::cov3d_decompose(cov, rot_xyzw, scale, [](float v) { return std::sqrt(v); });
}

extern "C" gs_status gs_decompose_pods(gs_sh_config src_sh, gs_cov3d_config src_cov, gs_sh_config dst_sh, const void *pods, size_t n,
                                       void *out) {
    if (src_cov == GS_COV3D_ROT_SCALE) return gs_convert_pods(src_sh, src_cov, dst_sh, GS_COV3D_ROT_SCALE, pods, n, out);
    if (!pods || !out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    if (!valid_cfg(src_sh, src_cov) || !valid_cfg(dst_sh, GS_COV3D_ROT_SCALE)) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "unknown layout config");
    const size_t ss = (size_t)gs::pod_bytes(src_sh, src_cov), ds = (size_t)gs::pod_bytes(dst_sh, gs::COV_ROT_SCALE);
    const uint8_t *in = (const uint8_t *)pods;
    uint8_t *o = (uint8_t *)out;
    for (size_t i = 0; i < n; i++) {
        uint32_t pw[56], ow[56];
        std::memcpy(pw, in + i * ss, ss);
        gs::decompose_words(src_sh, src_cov, dst_sh, pw, ow, [](float v) { return std::sqrt(v); });      // the same code the device kernel runs
        std::memcpy(o + i * ds, ow, ds);
    }
    return GS_OK;
}

// one kernel instance per pair of SH configs; the cov configs are kernel arguments
typedef void (*convert_fn)(const uint4 *, uint4 *, const uint32_t *, uint32_t, uint32_t, const uint32_t *, int, int, uint64_t, uint32_t);
#define GS_SH_ROW(s) {gs::k_convert_extract<s, 0>, gs::k_convert_extract<s, 1>, gs::k_convert_extract<s, 2>, gs::k_convert_extract<s, 3>}
static convert_fn k_tbl_convert[4][4] = {GS_SH_ROW(0), GS_SH_ROW(1), GS_SH_ROW(2), GS_SH_ROW(3)};
#undef GS_SH_ROW
typedef void (*decompose_fn)(const uint4 *, uint4 *, const uint32_t *, uint32_t, uint32_t, const uint32_t *, int, uint64_t, uint32_t);
#define GS_SH_ROW(s) {gs::k_decompose_extract<s, 0>, gs::k_decompose_extract<s, 1>, gs::k_decompose_extract<s, 2>, gs::k_decompose_extract<s, 3>}
static decompose_fn k_tbl_decompose[4][4] = {GS_SH_ROW(0), GS_SH_ROW(1), GS_SH_ROW(2), GS_SH_ROW(3)};
#undef GS_SH_ROW

// The `total` records the scan counted, converted: src (n records of layout (ssh, scov)) -> records [dst_base, dst_base +
// total) of dst (layout (dsh, dcov)), packed in index order.  A source that already has the destination layout is copied
// (k_extract_copy); a covariance source with a rot-scale destination (which only gs_gaussians_buffer_create_decomposed asks
// for) is decomposed.
static void convert_extract_enqueue(hipStream_t st, const gs_gaussians_buffer *src, int dsh, int dcov, void *dst, uint64_t dst_base,
                                    const uint32_t *words, uint32_t n, uint32_t invert, const uint32_t *offsets, uint32_t total) {
    if (dcov == gs::COV_ROT_SCALE && src->cov != gs::COV_ROT_SCALE) {
        hipLaunchKernelGGL(k_tbl_decompose[src->sh][dsh], dim3((n + 255u) / 256u), dim3(256), 0, st, (const uint4 *)src->buf->ptr,
                           (uint4 *)dst, words, n, invert, offsets, src->cov, dst_base, total);
        return;
    }
    if (src->sh == dsh && src->cov == dcov) {
        const uint32_t nc = (uint32_t)(pod_stride(src) / 16);
        extract_copy_enqueue(st, src->buf->ptr, (uint4 *)dst + dst_base * nc, words, n, invert, offsets, nc, total);
        return;
    }
    hipLaunchKernelGGL(k_tbl_convert[src->sh][dsh], dim3((n + 255u) / 256u), dim3(256), 0, st, (const uint4 *)src->buf->ptr, (uint4 *)dst,
                       words, n, invert, offsets, src->cov, dcov, dst_base, total);
}

gs_status gsh::extract_records(gs_gaussians_buffer *src, gs_stream *s, const gs_selection *sel, int32_t invert, int dsh, int dcov,
                               gs_gaussians_buffer **out, uint64_t *count_out, hipError_t *copy_error) {
    ExtractScan x;
    GS_TRY(extract_begin(src, s, sel, invert, x));
    gs_gaussians_buffer *dst = nullptr;
    if (x.total) {
        GS_TRY(gaussians_buffer_create_unfilled(x.dev, dsh, dcov, x.total, &dst));
        convert_extract_enqueue(x.st, src, dsh, dcov, dst->buf->ptr, 0, x.words, x.n, x.inv, x.offsets(), x.total);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(x.st);      // the offsets are freed with `x`; the call is blocking anyway
        if (e != hipSuccess) {
            gs_gaussians_buffer_destroy(dst);
            *copy_error = e;
            return GS_ERR_HIP;
        }
    } else {
        GS_TRY(gs_gaussians_buffer_create(x.dev, (gs_sh_config)dsh, (gs_cov3d_config)dcov, nullptr, 0, &dst));
    }
    dst->spatial = src->spatial;
    *out = dst;
    if (count_out) *count_out = x.total;
    return GS_OK;
}

extern "C" gs_status gs_gaussians_buffer_create_converted(gs_gaussians_buffer *src, gs_stream *s, const gs_selection *sel, int32_t invert,
                                                          gs_sh_config dst_sh, gs_cov3d_config dst_cov, gs_gaussians_buffer **out,
                                                          uint64_t *count_out) {
    if (out) *out = nullptr;
    if (!src || !out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    if (count_out) *count_out = 0;
    GS_TRY(check_pair(src->sh, src->cov, dst_sh, dst_cov));
    if (src->sh == (int)dst_sh && src->cov == (int)dst_cov) return gs_gaussians_buffer_create_from_selection(src, s, sel, invert, out, count_out);
    hipError_t e = hipSuccess;
    const gs_status rc = extract_records(src, s, sel, invert, dst_sh, dst_cov, out, count_out, &e);
    if (e != hipSuccess) return gs_fail(GS_ERR_HIP, (uint64_t)e, 0, 0, "conversion failed: %s", hipGetErrorString(e));
    return rc;
}

extern "C" gs_status gs_gaussians_buffer_create_decomposed(gs_gaussians_buffer *src, gs_stream *s, const gs_selection *sel, int32_t invert,
                                                           gs_sh_config dst_sh, gs_gaussians_buffer **out, uint64_t *count_out) {
    if (src && out && src->cov != gs::COV_ROT_SCALE) {
        *out = nullptr;
        if (count_out) *count_out = 0;
        if (!valid_cfg(dst_sh, GS_COV3D_ROT_SCALE)) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "unknown layout config");
        hipError_t e = hipSuccess;
        const gs_status rc = extract_records(src, s, sel, invert, dst_sh, gs::COV_ROT_SCALE, out, count_out, &e);
        if (e != hipSuccess) return gs_fail(GS_ERR_HIP, (uint64_t)e, 0, 0, "decomposition failed: %s", hipGetErrorString(e));
        return rc;
    }
    return gs_gaussians_buffer_create_converted(src, s, sel, invert, dst_sh, GS_COV3D_ROT_SCALE, out, count_out);
}

extern "C" gs_status gs_gaussians_buffer_create_concat_as(gs_stream *s, gs_gaussians_buffer *const *srcs, const gs_selection *const *sels,
                                                          uint32_t count, gs_sh_config dst_sh, gs_cov3d_config dst_cov,
                                                          gs_gaussians_buffer **out, uint64_t *counts_out) {
    return concat_records(s, srcs, sels, count, true, dst_sh, dst_cov, out, counts_out);
}

gs_status gsh::concat_records(gs_stream *s, gs_gaussians_buffer *const *srcs, const gs_selection *const *sels, uint32_t count, bool as_layout,
                              int dsh, int dcov, gs_gaussians_buffer **out, uint64_t *counts_out) {
    if (out) *out = nullptr;
    if (!srcs || !out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    if (count < 1u || count > 64u) return gs_fail(GS_ERR_INVALID_ARGUMENT, count, 0, 0, "a concatenation takes 1 to 64 sources, not %u", (unsigned)count);
    if (as_layout && !valid_cfg(dsh, dcov)) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "unknown layout config");
    if (counts_out) std::memset(counts_out, 0, (size_t)count * sizeof(uint64_t));
    size_t nblocks_all = 0;
    for (uint32_t i = 0; i < count; i++) {
        const gs_gaussians_buffer *g = srcs[i];
        if (!g) return gs_fail(GS_ERR_INVALID_ARGUMENT, i, 0, 0, "source %u is null", (unsigned)i);
        if (g->buf->dev != srcs[0]->buf->dev) return gs_fail(GS_ERR_INVALID_ARGUMENT, i, 0, 0, "objects belong to different devices");
        if (as_layout) {
            if (!gs::layout_convertible(g->sh, g->cov, dsh, dcov))
                return gs_fail(GS_ERR_LOSSY_CONFIG, i, 0, 0, "source %u: cannot convert a covariance back to rotation and scale", (unsigned)i);
        } else if (g->sh != srcs[0]->sh || g->cov != srcs[0]->cov) {
            return gs_fail(GS_ERR_INVALID_ARGUMENT, i, 0, 0, "source %u has another layout than source 0", (unsigned)i);
        }
        GS_TRY(check_buffer_selection(g, s, sels ? sels[i] : nullptr));
        const size_t len = gs_gaussians_buffer_len(g);
        GS_TRY(check_len32(len));
        nblocks_all += (len + gs::PLANAR_BLOCK - 1) / gs::PLANAR_BLOCK;
    }
    gs_device *dev = srcs[0]->buf->dev;
    const int sh = as_layout ? dsh : srcs[0]->sh, cov = as_layout ? dcov : srcs[0]->cov;
    GS_TRY(use_device(dev));
    hipStream_t st = stream_of(dev, s);
    // one array for all sources: the per-block offsets of source i from block0[i] on, then one total per source
    DevMem scan_mem;
    GS_TRY(scan_mem.alloc((nblocks_all + 64) * 4, 0, "hipMalloc"));
    uint32_t *scan = (uint32_t *)scan_mem.ptr, *totals_dev = scan + nblocks_all;
    uint32_t totals[64] = {};
    size_t block0[64] = {};
    hipError_t e = hipMemsetAsync(totals_dev, 0, 64 * 4, st);
    size_t b0 = 0;
    for (uint32_t i = 0; i < count && e == hipSuccess; i++) {
        gs_gaussians_buffer *g = srcs[i];
        const uint32_t n = (uint32_t)gs_gaussians_buffer_len(g);
        block0[i] = b0;
        b0 += (n + gs::PLANAR_BLOCK - 1u) / gs::PLANAR_BLOCK;
        if (!n) continue;
        GS_TRY(wait_for_edits(g, st));      // (scans of earlier sources may be in flight: the array's hipFree waits for them)
        extract_scan_enqueue(st, sels && sels[i] ? sels[i]->bits() : nullptr, n, 0u, scan + block0[i], totals_dev + i);
        e = hipGetLastError();
    }
    // sizing the new buffer needs the totals on the host: the one round trip of the call
    if (e == hipSuccess) e = fetch(st, totals, totals_dev, (size_t)count * 4);
    if (e != hipSuccess) return gs_fail(GS_ERR_HIP, (uint64_t)e, 0, 0, "selection scan failed: %s", hipGetErrorString(e));
    uint64_t total = 0;
    for (uint32_t i = 0; i < count; i++) {
        const size_t len = gs_gaussians_buffer_len(srcs[i]);
        if (totals[i] > len) return gs_fail(GS_ERR_HIP, totals[i], len, 0, "selection scan returned %u of %zu Gaussians", totals[i], len);
        total += totals[i];
    }
    if (total > 0xfffffff0ull)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, total, 0, 0, "the concatenation would hold %llu Gaussians", (unsigned long long)total);
    gs_gaussians_buffer *dst = nullptr;
    if (total) {
        GS_TRY(gaussians_buffer_create_unfilled(dev, sh, cov, (size_t)total, &dst));
        uint64_t first = 0;      // where the part of source i starts in the new buffer
        for (uint32_t i = 0; i < count; i++) {
            if (!totals[i]) continue;
            const uint32_t n = (uint32_t)gs_gaussians_buffer_len(srcs[i]);
            const uint32_t *words = sels && sels[i] ? sels[i]->bits() : nullptr;
            // both kernels stay inside `total` records from `first`: the part of this source
            convert_extract_enqueue(st, srcs[i], sh, cov, dst->buf->ptr, first, words, n, 0u, scan + block0[i], totals[i]);
            first += totals[i];
        }
        // The copies are only enqueued: the call has blocked once, for the totals.  The new buffer is ordered like an edited
        // one (frames, snapshots and extractions on other streams wait for the copies) and keeps the offsets they read.
        e = hipGetLastError();
        const gs_status rc = e != hipSuccess ? gs_fail(GS_ERR_HIP, (uint64_t)e, 0, 0, "concatenation failed: %s", hipGetErrorString(e))
                                             : record_edit(dst, st);
        if (rc != GS_OK) {
            (void)hipStreamSynchronize(st);      // the copies read the offsets, which are freed at the return
            gs_gaussians_buffer_destroy(dst);
            return rc;
        }
        dst->concat_offsets.ptr = scan_mem.release();
    } else {
        GS_TRY(gs_gaussians_buffer_create(dev, (gs_sh_config)sh, (gs_cov3d_config)cov, nullptr, 0, &dst));
    }
    dst->spatial = srcs[0]->spatial;
    *out = dst;
    if (counts_out)
        for (uint32_t i = 0; i < count; i++) counts_out[i] = totals[i];
    return GS_OK;
}
