// gs_neighbors.hip — neighbour counts and select by neighbourhood.  Kernels: gs_neighbor_kernels.h;
// the bounding-box reduction and the 64-bit sort are the render unit's (gs_host.h).
#include "gs_host.h"

#include "gs_neighbor_kernels.h"

using namespace gsh;

// ------------------------------------------------------------------------------------------------
// neighbour counts, select by neighbourhood
// ------------------------------------------------------------------------------------------------

gs_status gsh::check_neighbor_radius(float radius) {
    if (!(radius >= 0.0f) || !std::isfinite(radius) || !std::isfinite(radius * radius))
        return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "the radius must be finite and not negative, with a finite square");
    return GS_OK;
}

// The front of every call on the neighbour graph, on `st`: reserve, bounding box, keys, sort, gather.  n > 0, arguments
// checked.
gs_status gsh::neighbor_grid_enqueue(gs_gaussians_buffer *g, hipStream_t st, const gs_selection *among, const gs_model_transform_pod *mt,
                                     float radius, size_t extra_bytes, NeighborGrid &grid) {
    gs_device *dev = g->buf->dev;
    const uint32_t n = (uint32_t)gs_gaussians_buffer_len(g), pod_words = (uint32_t)(pod_stride(g) / 4);
    const uint32_t nblocks = (n + 255u) / 256u, pgrid = nblocks < 1024u ? nblocks : 1024u;
    // [keys 0][vals 0][keys 1][vals 1][count plane][bbox partials][bbox][extra]; the sorted positions (3 planes of n floats)
    // take the key / value pair the sort did not leave its result in
    const size_t a8 = ((size_t)n * 8 + 255) & ~(size_t)255, a4 = ((size_t)n * 4 + 255) & ~(size_t)255;
    const size_t part = ((size_t)pgrid * 24 + 255) & ~(size_t)255;
    GS_TRY(dev_reserve(g->nb_scratch, 2 * (a8 + a4) + a4 + part + 256 + extra_bytes));
    char *base = (char *)g->nb_scratch.ptr;
    void *k2[2] = {base, base + a8 + a4};
    void *v2[2] = {base + a8, base + 2 * a8 + a4};
    float *partial = (float *)(base + 2 * (a8 + a4) + a4), *bbox = (float *)(base + 2 * (a8 + a4) + a4 + part);
    // an edit enqueued on another stream still writes the records; a call on another stream still reads the scratch
    GS_TRY(wait_for_edits(g, st));
    if (g->nb_done && st != g->nb_stream) GS_HIP(hipStreamWaitEvent(st, g->nb_done, 0));
    gs::SelectShape sh{};
    gs_model_transform_pod def;
    if (!mt) {
        gs_model_transform_pod_default(&def);
        mt = &def;
    }
    gs::ModelTransform m;
    std::memcpy(&m, mt, sizeof(m));
    gs::model_transform_mat(m, sh.M);
    const uint32_t *aos = (const uint32_t *)g->buf->ptr, *words = among ? among->bits() : nullptr;
    hipLaunchKernelGGL(gs::k_nb_bbox_partial, dim3(pgrid), dim3(256), 0, st, aos, pod_words, n, words, sh, partial);
    bbox_final_enqueue(st, partial, pgrid, bbox);
    hipLaunchKernelGGL(gs::k_nb_keys, dim3(nblocks), dim3(256), 0, st, aos, pod_words, n, words, sh, (const float *)bbox, radius,
                       (uint64_t *)k2[0], (uint32_t *)v2[0]);
    GS_HIP(hipGetLastError());
    int side = 0;
    uint32_t passes = 0;
    GS_TRY(sort_pairs_device<uint64_t>(dev, k2, v2, g->nb_ghist, g->nb_digit_totals, n, 64, st, side, passes));
    const uint64_t *skeys = (const uint64_t *)k2[side];
    const uint32_t *svals = (const uint32_t *)v2[side];
    float *sx = (float *)k2[side ^ 1], *sy = sx + n, *sz = sy + n;      // 12 n bytes <= a8 + a4, the pair is contiguous
    hipLaunchKernelGGL(gs::k_nb_gather, dim3(nblocks), dim3(256), 0, st, aos, pod_words, n, sh, skeys, svals, sx, sy, sz);
    GS_HIP(hipGetLastError());
    grid.keys = skeys;
    grid.vals = svals;
    grid.sx = sx;
    grid.sy = sy;
    grid.sz = sz;
    grid.bbox = bbox;
    grid.plane = (uint32_t *)(base + 2 * (a8 + a4));
    grid.extra = base + 2 * (a8 + a4) + a4 + part + 256;
    grid.n = n;
    grid.nblocks = nblocks;
    return GS_OK;
}

// counts[i] = min(c_i, cap) in caller order on `st` (mark: gs::NB_NOT_A_POINT where i is no point); counts == nullptr: the
// plane of the buffer's scratch, returned in *plane_out.  n > 0, arguments checked.
static gs_status neighbor_counts_enqueue(gs_gaussians_buffer *g, hipStream_t st, const gs_selection *among,
                                         const gs_model_transform_pod *mt, float radius, uint32_t cap, bool mark, uint32_t *counts,
                                         uint32_t **plane_out) {
    NeighborGrid q;
    GS_TRY(neighbor_grid_enqueue(g, st, among, mt, radius, 0, q));
    if (!counts) counts = q.plane;
    const float rr = radius * radius;
    if (mark)
        hipLaunchKernelGGL(gs::k_nb_count<true>, dim3(q.nblocks), dim3(256), 0, st, q.keys, q.vals, q.sx, q.sy, q.sz, q.n, rr, cap, counts);
    else
        hipLaunchKernelGGL(gs::k_nb_count<false>, dim3(q.nblocks), dim3(256), 0, st, q.keys, q.vals, q.sx, q.sy, q.sz, q.n, rr, cap, counts);
    GS_HIP(hipGetLastError());
    if (plane_out) *plane_out = q.plane;
    return GS_OK;
}

// the next call on another stream waits until this one has left the scratch
gs_status gsh::neighbor_scratch_release(gs_gaussians_buffer *g, hipStream_t st) {
    if (!g->nb_done) GS_HIP_AS("hipEventCreateWithFlags(&g->nb_done, hipEventDisableTiming)", g->nb_done.create());
    GS_HIP(hipEventRecord(g->nb_done, st));
    g->nb_stream = st;
    return GS_OK;
}

extern "C" gs_status gs_gaussians_buffer_neighbor_counts(gs_gaussians_buffer *g, gs_stream *s, const gs_selection *among,
                                                         const gs_model_transform_pod *mt, float radius, uint32_t cap,
                                                         gs_buffer *counts_out) {
    if (!g || !counts_out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    GS_TRY(check_neighbor_radius(radius));
    if (!cap) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "cap must be at least 1");
    RecordsAccess r;
    GS_TRY(records_check(g, s, among, 0, r));
    const size_t len = r.len;
    if (counts_out->dev != g->buf->dev) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "objects belong to different devices");
    if (counts_out->bytes < len * 4)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, counts_out->bytes, len * 4, 0, "the count plane has %zu bytes, %zu Gaussians need %zu",
                    counts_out->bytes, len, len * 4);
    if (!len) return GS_OK;
    GS_TRY(use_device(r.dev));
    hipStream_t st = stream_of(r.dev, s);
    // the event on every path: an enqueue that failed half-way has still left kernels on the scratch
    const gs_status rc = neighbor_counts_enqueue(g, st, among, mt, radius, cap, false, (uint32_t *)counts_out->ptr, nullptr);
    const gs_status ev = neighbor_scratch_release(g, st);
    return rc != GS_OK ? rc : ev;
}

extern "C" gs_status gs_select_neighbors(gs_selection *sel, gs_stream *s, gs_gaussians_buffer *g, const gs_selection *among,
                                         const gs_model_transform_pod *mt, float radius, uint32_t min_count, uint32_t max_count,
                                         gs_select_op op) {
    if (!sel || !g) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    GS_TRY(check_select_op(op));
    GS_TRY(check_neighbor_radius(radius));
    if (g->buf->dev != sel->dev) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "objects belong to different devices");
    GS_TRY(check_buffer_selection(g, s, among));
    const size_t len = gs_gaussians_buffer_len(g);
    if (len != sel->n) return gs_fail(GS_ERR_INVALID_ARGUMENT, sel->n, len, 0, "the selection has %zu bits, the buffer %zu Gaussians", sel->n, len);
    GS_TRY(check_len32(len));
    gs_device *dev = sel->dev;
    GS_TRY(use_device(dev));
    hipStream_t st = stream_of(dev, s);
    if (!len) {
        sel->generation = next_object_id();
        return GS_OK;
    }
    const uint32_t n = (uint32_t)len;
    if (min_count > max_count) {      // sel = sel op {}
        sel->generation = next_object_id();
        sel_range_enqueue(sel, st, 0u, 0u, op);
        GS_HIP(hipGetLastError());
        return GS_OK;
    }
    // a count above max_count only has to be known as such
    const uint32_t cap = max_count == 0xffffffffu ? max_count : max_count + 1u;
    uint32_t *plane = nullptr;
    gs_status rc = neighbor_counts_enqueue(g, st, among, mt, radius, cap, true, nullptr, &plane);
    if (rc == GS_OK) {      // only now does `sel` change
        sel->generation = next_object_id();
        hipLaunchKernelGGL(gs::k_nb_select, dim3((n + 255u) / 256u), dim3(256), 0, st, (const uint32_t *)plane, n, min_count, max_count,
                           sel->bits(), (uint32_t)op);
        if (hipGetLastError() != hipSuccess) rc = gs_fail(GS_ERR_HIP, 0, 0, 0, "k_nb_select could not be launched");
    }
    // the event on every path: an enqueue that failed half-way has still left kernels on the scratch
    const gs_status ev = neighbor_scratch_release(g, st);
    return rc != GS_OK ? rc : ev;
}
