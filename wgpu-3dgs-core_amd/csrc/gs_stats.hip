// gs_stats.hip — the read side of the device editor: attribute statistics, histograms, select by
// attribute range.  Kernels: gs_stats_kernels.h.
#include "gs_host.h"

#include "gs_stats_kernels.h"

using namespace gsh;

// ------------------------------------------------------------------------------------------------
// attribute statistics, histograms, select by attribute range
// ------------------------------------------------------------------------------------------------

#define GS_ATTR_COV_TABLE(kernel)                                                                                       \
    {                                                                                                                   \
        {kernel<gs::ATTR_CLASS_COV, 0, 0>, kernel<gs::ATTR_CLASS_COV, 0, 1>, kernel<gs::ATTR_CLASS_COV, 0, 2>},         \
        {kernel<gs::ATTR_CLASS_COV, 1, 0>, kernel<gs::ATTR_CLASS_COV, 1, 1>, kernel<gs::ATTR_CLASS_COV, 1, 2>},         \
        {kernel<gs::ATTR_CLASS_COV, 2, 0>, kernel<gs::ATTR_CLASS_COV, 2, 1>, kernel<gs::ATTR_CLASS_COV, 2, 2>},         \
        {kernel<gs::ATTR_CLASS_COV, 3, 0>, kernel<gs::ATTR_CLASS_COV, 3, 1>, kernel<gs::ATTR_CLASS_COV, 3, 2>},         \
    }

typedef void (*select_attr_fn)(const uint32_t *, uint32_t, uint32_t, gs::AttrArgs, float, float, uint32_t *, uint32_t);
typedef void (*histogram_fn)(const uint32_t *, uint32_t, uint32_t, const uint32_t *, gs::AttrArgs, float, float, float, uint32_t,
                             unsigned long long *);
typedef void (*stats_fn)(const uint32_t *, uint32_t, const uint32_t *, gs::AttrArgs, uint32_t *, double *, uint32_t);
static select_attr_fn k_tbl_select_attr_cov[4][3] = GS_ATTR_COV_TABLE(gs::k_select_attr);
static histogram_fn k_tbl_histogram_cov[4][3] = GS_ATTR_COV_TABLE(gs::k_histogram);
static stats_fn k_tbl_stats[4][3] = GS_CFG_TABLE(gs::k_stats_partial);

// the kernel of an attribute's class: the position and colour passes do not depend on the layout
static select_attr_fn select_attr_kernel(const gs_gaussians_buffer *g, uint32_t attr) {
    const int cls = gs::attr_class(attr);
    return cls == gs::ATTR_CLASS_POS ? gs::k_select_attr<gs::ATTR_CLASS_POS, 0, 0>
           : cls == gs::ATTR_CLASS_COLOR ? gs::k_select_attr<gs::ATTR_CLASS_COLOR, 0, 0> : k_tbl_select_attr_cov[g->sh][g->cov];
}
static histogram_fn histogram_kernel(const gs_gaussians_buffer *g, uint32_t attr) {
    const int cls = gs::attr_class(attr);
    return cls == gs::ATTR_CLASS_POS ? gs::k_histogram<gs::ATTR_CLASS_POS, 0, 0>
           : cls == gs::ATTR_CLASS_COLOR ? gs::k_histogram<gs::ATTR_CLASS_COLOR, 0, 0> : k_tbl_histogram_cov[g->sh][g->cov];
}

// the constants of an attribute pass; NULL transform = the default one through the same arithmetic
static void attr_args_fill(gs::AttrArgs &a, uint32_t attr, const gs_model_transform_pod *mt, const float *ref) {
    gs_model_transform_pod def;
    if (!mt) {
        gs_model_transform_pod_default(&def);
        mt = &def;
    }
    gs::ModelTransform m;
    std::memcpy(&m, mt, sizeof(m));
    gs::model_transform_mat(m, a.M);
    for (int k = 0; k < 3; k++) a.ref[k] = ref ? ref[k] : 0.0f;
    a.attr = attr;
}

static gs_status check_attribute_desc(const gs_attribute_desc *a) {
    if (!a) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    if (a->attr >= (uint32_t)GS_ATTR_COUNT) return gs_fail(GS_ERR_INVALID_ARGUMENT, a->attr, 0, 0, "unknown attribute %u", (unsigned)a->attr);
    for (uint32_t r : a->reserved)
        if (r) return gs_fail(GS_ERR_INVALID_ARGUMENT, r, 0, 0, "gs_attribute_desc.reserved must be 0");
    if (a->attr == (uint32_t)GS_ATTR_DIST2 && !all_finite(a->ref, 3))
        return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "the reference point of GS_ATTR_DIST2 must be finite");
    return GS_OK;
}

extern "C" gs_status gs_gaussians_buffer_stats(gs_gaussians_buffer *g, gs_stream *s, const gs_selection *sel,
                                               const gs_model_transform_pod *mt, const float ref[3], gs_stats *out) {
    if (!g || !out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    if (ref && !all_finite(ref, 3)) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "the reference point must be finite");
    RecordsAccess r;
    GS_TRY(records_check(g, s, sel, 0, r));
    const size_t len = r.len;
    static_assert(sizeof(gs::StatsOut) == sizeof(gs_stats), "the device result is a gs_stats");
    gs_stats res;
    std::memset(&res, 0, sizeof(res));
    for (gs_attribute_stats &a : res.attr) {
        a.min = INFINITY;
        a.max = -INFINITY;
    }
    if (len) {
        // (the scratch grows before the wait for edits, as it always did: the second half of records_access by hand)
        GS_TRY(use_device(r.dev));
        hipStream_t st = stream_of(r.dev, s);
        const uint32_t n = r.n, nblocks = (n + 255u) / 256u;
        // [the result, 256 bytes][the sums: 9 x nblocks doubles][the integer fields: 28 x nblocks words]
        const size_t d_bytes = (size_t)gs::ATTR_COUNT * nblocks * 8, u_bytes = (size_t)gs::STATS_U_FIELDS * nblocks * 4;
        GS_TRY(dev_reserve(g->stats_scratch, 256 + d_bytes + u_bytes));
        // an edit enqueued on another stream still writes the records
        GS_TRY(wait_for_edits(g, st));
        gs::StatsOut *dout = (gs::StatsOut *)g->stats_scratch.ptr;
        double *part_d = (double *)((char *)g->stats_scratch.ptr + 256);
        uint32_t *part_u = (uint32_t *)((char *)g->stats_scratch.ptr + 256 + d_bytes);
        gs::AttrArgs a;
        attr_args_fill(a, 0u, mt, ref);
        hipLaunchKernelGGL(k_tbl_stats[g->sh][g->cov], dim3(nblocks), dim3(256), 0, st, (const uint32_t *)g->buf->ptr, n,
                           r.words, a, part_u, part_d, nblocks);
        hipLaunchKernelGGL(gs::k_stats_finish, dim3(1), dim3(256), 0, st, (const uint32_t *)part_u, (const double *)part_d, nblocks, dout);
        GS_HIP(hipGetLastError());
        GS_HIP(hipMemcpyAsync(&res, dout, sizeof(res), hipMemcpyDeviceToHost, st));
        hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) return gs_fail(GS_ERR_DOWNLOAD, (uint64_t)e, 0, 0, "download failed: %s", hipGetErrorString(e));
    }
    *out = res;
    return GS_OK;
}

extern "C" gs_status gs_gaussians_buffer_histogram(gs_gaussians_buffer *g, gs_stream *s, const gs_selection *sel,
                                                   const gs_attribute_desc *ad, float lo, float hi, uint32_t bins, uint64_t *counts_out) {
    if (!g || !counts_out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    GS_TRY(check_attribute_desc(ad));
    if (bins < 1u || bins > 4096u) return gs_fail(GS_ERR_INVALID_ARGUMENT, bins, 0, 0, "a histogram takes 1 to 4096 bins, not %u", (unsigned)bins);
    const float width = hi - lo;
    if (!std::isfinite(lo) || !std::isfinite(hi) || !std::isfinite(width) || !(hi > lo))
        return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "the range of a histogram must be finite, with hi > lo");
    const float scale = (float)bins / width;
    if (!std::isfinite(scale)) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "bins / (hi - lo) is not finite in binary32");
    RecordsAccess r;
    GS_TRY(records_check(g, s, sel, 0, r));
    const size_t len = r.len;
    const size_t slots = 2 * ((size_t)bins + 3);
    if (!len) {
        std::memset(counts_out, 0, slots * sizeof(uint64_t));
        return GS_OK;
    }
    GS_TRY(use_device(r.dev));
    hipStream_t st = stream_of(r.dev, s);
    GS_TRY(dev_reserve(g->stats_scratch, slots * 8));
    // an edit enqueued on another stream still writes the records
    GS_TRY(wait_for_edits(g, st));
    GS_HIP(hipMemsetAsync(g->stats_scratch.ptr, 0, slots * 8, st));
    gs::AttrArgs a;
    attr_args_fill(a, ad->attr, ad->model_transform, ad->ref);
    const uint32_t n = r.n, nblocks = (n + 255u) / 256u, grid = nblocks < 2048u ? nblocks : 2048u;
    hipLaunchKernelGGL(histogram_kernel(g, ad->attr), dim3(grid), dim3(256), slots * 4, st, (const uint32_t *)g->buf->ptr,
                       (uint32_t)(pod_stride(g) / 4), n, r.words, a, lo, hi, scale, bins,
                       (unsigned long long *)g->stats_scratch.ptr);
    GS_HIP(hipGetLastError());
    // into a host copy first: counts_out stays untouched when the stream reports a failure
    std::vector<uint64_t> host(slots);
    GS_HIP(hipMemcpyAsync(host.data(), g->stats_scratch.ptr, slots * 8, hipMemcpyDeviceToHost, st));
    hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return gs_fail(GS_ERR_DOWNLOAD, (uint64_t)e, 0, 0, "download failed: %s", hipGetErrorString(e));
    std::memcpy(counts_out, host.data(), slots * 8);
    return GS_OK;
}

extern "C" gs_status gs_select_attribute(gs_selection *sel, gs_stream *s, gs_gaussians_buffer *g, const gs_attribute_desc *ad, float lo,
                                         float hi, gs_select_op op) {
    GS_TRY(check_selection(sel, s));
    GS_TRY(check_select_op(op));
    if (!g) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    GS_TRY(check_attribute_desc(ad));
    if (lo != lo || hi != hi) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "a bound of the range is NaN");
    if (g->buf->dev != sel->dev) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "objects belong to different devices");
    const size_t len = gs_gaussians_buffer_len(g);
    if (len != sel->n) return gs_fail(GS_ERR_INVALID_ARGUMENT, sel->n, len, 0, "the selection has %zu bits, the buffer %zu Gaussians", sel->n, len);
    GS_TRY(check_len32(len));
    sel->generation = next_object_id();
    if (!len) return GS_OK;
    // an edit enqueued on another stream still writes the records
    GS_TRY(wait_for_edits(g, s->s));
    gs::AttrArgs a;
    attr_args_fill(a, ad->attr, ad->model_transform, ad->ref);
    const uint32_t n = (uint32_t)len;
    hipLaunchKernelGGL(select_attr_kernel(g, ad->attr), dim3((n + 255u) / 256u), dim3(256), 0, s->s, (const uint32_t *)g->buf->ptr,
                       (uint32_t)(pod_stride(g) / 4), n, a, lo, hi, sel->bits(), (uint32_t)op);
    GS_HIP(hipGetLastError());
    return GS_OK;
}
