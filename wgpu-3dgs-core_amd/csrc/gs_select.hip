// gs_select.hip — Gaussian selections: create / combine / upload / download / count, select by sphere,
// box and range, and the argument checks the other units share.  Kernels: gs_select_kernels.h.
#include "gs_host.h"

#include "gs_select_kernels.h"

using namespace gsh;

// ------------------------------------------------------------------------------------------------
// Gaussian selections
// ------------------------------------------------------------------------------------------------

extern "C" gs_status gs_selection_create(gs_device *dev, size_t n, gs_selection **out) {
    if (!dev || !out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    GS_TRY(check_len32(n));
    GS_TRY(use_device(dev));
    const size_t nwords = (n + 31) / 32, bytes = (nwords ? nwords : 1) * 4;
    std::unique_ptr<gs_selection> sel(new gs_selection());
    GS_TRY(sel->words.alloc(bytes, 0, "selection allocation"));
    hipError_t e = hipMemset(sel->words.ptr, 0, bytes);
    // (awaited: the null stream's fill is not ordered against the non-blocking stream of the upload that follows, and a
    // late fill clears a mask that was uploaded and already read once)
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess)
        return gs_fail(e == hipErrorOutOfMemory ? GS_ERR_OUT_OF_MEMORY : GS_ERR_HIP, (uint64_t)e, 0, 0, "selection allocation failed: %s",
                    hipGetErrorString(e));
    sel->dev = dev;
    sel->n = n;
    sel->nwords = nwords;
    sel->generation = next_object_id();
    *out = sel.release();
    return GS_OK;
}

extern "C" void gs_selection_destroy(gs_selection *sel) {
    if (!sel) return;
    (void)hipSetDevice(sel->dev->ordinal);
    delete sel;      // (hipFree synchronises the device: kernels that still read the mask finish first)
}

extern "C" size_t gs_selection_len(const gs_selection *sel) { return sel ? sel->n : 0; }

gs_status gsh::check_selection(const gs_selection *sel, const gs_stream *s) {
    if (!sel || !s) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    if (s->dev != sel->dev) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "objects belong to different devices");
    return use_device(sel->dev);
}
gs_status gsh::check_select_op(gs_select_op op) {
    if ((uint32_t)op > (uint32_t)GS_SEL_XOR) return gs_fail(GS_ERR_INVALID_ARGUMENT, (uint64_t)op, 0, 0, "unknown gs_select_op %u", (unsigned)op);
    return GS_OK;
}

gs_status gsh::check_buffer_selection(const gs_gaussians_buffer *g, const gs_stream *s, const gs_selection *sel) {
    if (s && s->dev != g->buf->dev) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "objects belong to different devices");
    if (!sel) return GS_OK;
    if (sel->dev != g->buf->dev) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "objects belong to different devices");
    const size_t len = gs_gaussians_buffer_len(g);
    if (sel->n != len) return gs_fail(GS_ERR_INVALID_ARGUMENT, sel->n, len, 0, "the selection has %zu bits, the buffer %zu Gaussians", sel->n, len);
    return GS_OK;
}

static gs_status selection_unary(gs_selection *sel, gs_stream *s, uint32_t mode) {
    GS_TRY(check_selection(sel, s));
    sel->generation = next_object_id();
    if (!sel->nwords) return GS_OK;
    hipLaunchKernelGGL(gs::k_sel_unary, dim3(sel->grid()), dim3(256), 0, s->s, sel->bits(), (uint32_t)sel->nwords, sel->tail_mask(), mode);
    GS_HIP(hipGetLastError());
    return GS_OK;
}
extern "C" gs_status gs_selection_clear(gs_selection *sel, gs_stream *s) { return selection_unary(sel, s, 0u); }
extern "C" gs_status gs_selection_fill(gs_selection *sel, gs_stream *s) { return selection_unary(sel, s, 1u); }
extern "C" gs_status gs_selection_invert(gs_selection *sel, gs_stream *s) { return selection_unary(sel, s, 2u); }

gs_status gsh::selection_combine_words(gs_selection *dst, hipStream_t st, gs_select_op op, const uint32_t *src) {
    dst->generation = next_object_id();
    if (!dst->nwords) return GS_OK;
    hipLaunchKernelGGL(gs::k_sel_combine, dim3(dst->grid()), dim3(256), 0, st, dst->bits(), src, (uint32_t)dst->nwords, (uint32_t)op);
    GS_HIP(hipGetLastError());
    return GS_OK;
}

extern "C" gs_status gs_selection_combine(gs_selection *dst, gs_stream *s, gs_select_op op, const gs_selection *src) {
    GS_TRY(check_selection(dst, s));
    GS_TRY(check_select_op(op));
    if (!src || src->dev != dst->dev) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "the source selection is null or belongs to another device");
    if (src->n != dst->n) return gs_fail(GS_ERR_INVALID_ARGUMENT, src->n, dst->n, 0, "selection lengths differ: %zu != %zu", src->n, dst->n);
    return selection_combine_words(dst, s->s, op, src->bits());
}

extern "C" gs_status gs_selection_upload(gs_selection *sel, gs_stream *s, const uint32_t *words, size_t nwords) {
    GS_TRY(check_selection(sel, s));
    if (nwords != sel->nwords || (nwords && !words))
        return gs_fail(GS_ERR_INVALID_ARGUMENT, nwords, sel->nwords, 0, "a selection of %zu bits takes %zu words", sel->n, sel->nwords);
    sel->generation = next_object_id();
    if (!nwords) return GS_OK;
    GS_HIP(hipMemcpyAsync(sel->bits(), words, nwords * 4, hipMemcpyHostToDevice, s->s));
    return selection_unary(sel, s, 3u);      // bits past n of the last word are dropped
}

extern "C" gs_status gs_selection_download(gs_selection *sel, gs_stream *s, uint32_t *words, size_t nwords) {
    GS_TRY(check_selection(sel, s));
    if (nwords != sel->nwords || (nwords && !words))
        return gs_fail(GS_ERR_INVALID_ARGUMENT, nwords, sel->nwords, 0, "a selection of %zu bits takes %zu words", sel->n, sel->nwords);
    if (!nwords) return GS_OK;
    GS_HIP(hipStreamSynchronize(s->s));
    hipError_t e = hipMemcpy(words, sel->bits(), nwords * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return gs_fail(GS_ERR_DOWNLOAD, (uint64_t)e, 0, 0, "download failed: %s", hipGetErrorString(e));
    return GS_OK;
}

extern "C" gs_status gs_selection_count(gs_selection *sel, gs_stream *s, uint64_t *out) {
    GS_TRY(check_selection(sel, s));
    if (!out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null out");
    *out = 0;
    if (!sel->nwords) return GS_OK;
    GS_TRY(dev_reserve(sel->counter, 8));
    GS_HIP(hipMemsetAsync(sel->counter.ptr, 0, 8, s->s));
    hipLaunchKernelGGL(gs::k_sel_count, dim3(sel->grid()), dim3(256), 0, s->s, sel->bits(), (uint32_t)sel->nwords,
                       (unsigned long long *)sel->counter.ptr);
    GS_HIP(hipGetLastError());
    GS_HIP(hipStreamSynchronize(s->s));
    hipError_t e = hipMemcpy(out, sel->counter.ptr, 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return gs_fail(GS_ERR_DOWNLOAD, (uint64_t)e, 0, 0, "download failed: %s", hipGetErrorString(e));
    return GS_OK;
}

// sphere / box: one thread per Gaussian of the AoS buffer, which is always current (the mirror is not needed)
static gs_status select_shape(gs_selection *sel, gs_stream *s, gs_gaussians_buffer *g, const gs_model_transform_pod *mt, bool box,
                              const float *params, gs_select_op op) {
    GS_TRY(check_selection(sel, s));
    GS_TRY(check_select_op(op));
    if (!g || !mt || !params) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    if (g->buf->dev != sel->dev) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "objects belong to different devices");
    const size_t len = gs_gaussians_buffer_len(g);
    if (len != sel->n) return gs_fail(GS_ERR_INVALID_ARGUMENT, sel->n, len, 0, "the selection has %zu bits, the buffer %zu Gaussians", sel->n, len);
    gs::SelectShape sh;
    gs::ModelTransform m;
    std::memcpy(&m, mt, sizeof(m));
    gs::model_transform_mat(m, sh.M);
    std::memcpy(sh.P, params, 12 * sizeof(float));
    sel->generation = next_object_id();
    if (!len) return GS_OK;
    const uint32_t n = (uint32_t)len, grid = (n + 255u) / 256u, pod_words = (uint32_t)(pod_stride(g) / 4);
    if (box)
        hipLaunchKernelGGL(gs::k_select_shape<true>, dim3(grid), dim3(256), 0, s->s, (const uint32_t *)g->buf->ptr, pod_words, n, sh, sel->bits(),
                           (uint32_t)op);
    else
        hipLaunchKernelGGL(gs::k_select_shape<false>, dim3(grid), dim3(256), 0, s->s, (const uint32_t *)g->buf->ptr, pod_words, n, sh, sel->bits(),
                           (uint32_t)op);
    GS_HIP(hipGetLastError());
    return GS_OK;
}

extern "C" gs_status gs_select_sphere(gs_selection *sel, gs_stream *s, gs_gaussians_buffer *g, const gs_model_transform_pod *mt,
                                      const float center[3], float radius, gs_select_op op) {
    if (!center) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    if (!(radius >= 0.0f)) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "the radius must be >= 0");
    float p[12] = {center[0], center[1], center[2], radius * radius};
    return select_shape(sel, s, g, mt, false, p, op);
}

extern "C" gs_status gs_select_box(gs_selection *sel, gs_stream *s, gs_gaussians_buffer *g, const gs_model_transform_pod *mt,
                                   const float world_to_box[12], gs_select_op op) {
    return select_shape(sel, s, g, mt, true, world_to_box, op);
}

// the caller's contribution records: n x 16 bytes, 16-byte aligned, on `dev`
gs_status gsh::check_contrib_buffer(const gs_buffer *contrib, const gs_device *dev, size_t n) {
    if (!contrib || !contrib->ptr) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    if (contrib->dev != dev) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "objects belong to different devices");
    if (n > contrib->bytes / sizeof(gs_contribution))
        return gs_fail(GS_ERR_INVALID_ARGUMENT, contrib->bytes, n, 0, "the contribution buffer holds %zu bytes, %zu records need %zu", contrib->bytes, n,
                       n * sizeof(gs_contribution));
    if ((uintptr_t)contrib->ptr & 15u)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, (uint64_t)(uintptr_t)contrib->ptr, 16, 0, "the contribution records must be 16-byte aligned");
    return GS_OK;
}

extern "C" gs_status gs_contributions_clear(gs_buffer *contrib, gs_stream *s, size_t n) {
    if (!contrib || !s) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    GS_TRY(check_contrib_buffer(contrib, s->dev, n));
    GS_TRY(use_device(s->dev));
    if (!n) return GS_OK;
    GS_HIP(hipMemsetAsync(contrib->ptr, 0, n * sizeof(gs_contribution), s->s));
    return GS_OK;
}

extern "C" gs_status gs_select_contribution(gs_selection *sel, gs_stream *s, gs_buffer *contrib, uint32_t kind, float lo, float hi,
                                            gs_select_op op) {
    GS_TRY(check_selection(sel, s));
    GS_TRY(check_select_op(op));
    if (kind > (uint32_t)GS_CONTRIB_MAX) return gs_fail(GS_ERR_INVALID_ARGUMENT, kind, 0, 0, "unknown contribution kind %u", (unsigned)kind);
    if (lo != lo || hi != hi) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "a bound of the range is NaN");
    GS_TRY(check_len32(sel->n));
    GS_TRY(check_contrib_buffer(contrib, sel->dev, sel->n));
    sel->generation = next_object_id();
    if (!sel->n) return GS_OK;
    const uint32_t n = (uint32_t)sel->n;
    hipLaunchKernelGGL(gs::k_select_contrib, dim3((n + 255u) / 256u), dim3(256), 0, s->s, (const uint4 *)contrib->ptr, n, kind, lo, hi, sel->bits(),
                       (uint32_t)op);
    GS_HIP(hipGetLastError());
    return GS_OK;
}

void gsh::sel_range_enqueue(gs_selection *sel, hipStream_t st, uint32_t start, uint32_t end, gs_select_op op) {
    hipLaunchKernelGGL(gs::k_sel_range, dim3(sel->grid()), dim3(256), 0, st, sel->bits(), (uint32_t)sel->nwords, start, end, (uint32_t)op);
}

extern "C" gs_status gs_select_range(gs_selection *sel, gs_stream *s, size_t start, size_t count, gs_select_op op) {
    GS_TRY(check_selection(sel, s));
    GS_TRY(check_select_op(op));
    if (start + count < start || start + count > sel->n)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, start, count, sel->n, "the range [%zu, %zu + %zu) leaves a selection of %zu bits", start, start, count, sel->n);
    sel->generation = next_object_id();
    if (!sel->nwords) return GS_OK;
    sel_range_enqueue(sel, s->s, (uint32_t)start, (uint32_t)(start + count), op);
    GS_HIP(hipGetLastError());
    return GS_OK;
}
