// gs_components.hip — connected components of the neighbour graph and the selects by cluster.  Kernels:
// gs_component_kernels.h; the grid, the sort and the sorted positions are the front of gs_neighbors.hip (gs_host.h).
#include "gs_host.h"

#include "gs_component_kernels.h"

using namespace gsh;

// ------------------------------------------------------------------------------------------------
// components, select by cluster size, select connected
// ------------------------------------------------------------------------------------------------

static_assert(sizeof(gs_components_info) == 16, "gs_components_info is four words");

// Behind the shared front on `st`: init, link, finalise, then the caller-order planes.  labels / sizes / info: where L, S
// and the info go (each may be null); seeds: the mask of gs_select_connected, then `sizes` receives 1 where the component
// of i holds a seed and 0 elsewhere.  sizes == nullptr with want_plane: the plane of the buffer's scratch, returned in
// *plane_out.  n > 0, arguments checked.
static gs_status components_enqueue(gs_gaussians_buffer *g, hipStream_t st, const gs_selection *among, const gs_model_transform_pod *mt,
                                    float radius, uint32_t *labels, uint32_t *sizes, uint32_t *info, const uint32_t *seeds,
                                    uint32_t **plane_out) {
    const size_t n4 = ((size_t)gs_gaussians_buffer_len(g) * 4 + 255) & ~(size_t)255;
    NeighborGrid q;
    // [parent][root][smallest index per root][points per root, or its seed flag]
    GS_TRY(neighbor_grid_enqueue(g, st, among, mt, radius, 4 * n4, q));
    char *extra = (char *)q.extra;
    uint32_t *parent = (uint32_t *)extra, *root = (uint32_t *)(extra + n4), *rootmin = (uint32_t *)(extra + 2 * n4),
             *rootsize = (uint32_t *)(extra + 3 * n4);
    if (plane_out) {
        sizes = q.plane;
        *plane_out = q.plane;
    }
    const dim3 grid(q.nblocks), block(256);
    hipLaunchKernelGGL(gs::k_cc_init, grid, block, 0, st, q.n, parent, rootmin, rootsize, info);
    hipLaunchKernelGGL(gs::k_cc_link, grid, block, 0, st, q.keys, q.sx, q.sy, q.sz, q.n, radius * radius, parent);
    if (seeds)
        hipLaunchKernelGGL(gs::k_cc_finalise<true>, grid, block, 0, st, q.keys, q.vals, (const uint32_t *)parent, q.n, root, rootmin,
                           rootsize, seeds);
    else
        hipLaunchKernelGGL(gs::k_cc_finalise<false>, grid, block, 0, st, q.keys, q.vals, (const uint32_t *)parent, q.n, root, rootmin,
                           rootsize, seeds);
    hipLaunchKernelGGL(gs::k_cc_scatter, grid, block, 0, st, q.keys, q.vals, (const uint32_t *)root, (const uint32_t *)rootmin,
                       (const uint32_t *)rootsize, q.n, labels, sizes, info);
    if (info)
        hipLaunchKernelGGL(gs::k_cc_largest_label, grid, block, 0, st, q.keys, (const uint32_t *)root, (const uint32_t *)rootmin,
                           (const uint32_t *)rootsize, q.n, info);
    GS_HIP(hipGetLastError());
    return GS_OK;
}

static gs_status check_component_plane(const gs_buffer *b, const gs_device *dev, size_t need, const char *what) {
    if (!b) return GS_OK;
    if (b->dev != dev) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "objects belong to different devices");
    if (b->bytes < need)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, b->bytes, need, 0, "the %s buffer has %zu bytes, %zu are needed", what, b->bytes, need);
    return GS_OK;
}

extern "C" gs_status gs_gaussians_buffer_components(gs_gaussians_buffer *g, gs_stream *s, const gs_selection *among,
                                                    const gs_model_transform_pod *mt, float radius, gs_buffer *labels_out,
                                                    gs_buffer *sizes_out, gs_buffer *info_out) {
    if (!g || (!labels_out && !sizes_out && !info_out)) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    GS_TRY(check_neighbor_radius(radius));
    RecordsAccess r;
    GS_TRY(records_check(g, s, among, 0, r));
    GS_TRY(check_component_plane(labels_out, g->buf->dev, r.len * 4, "label"));
    GS_TRY(check_component_plane(sizes_out, g->buf->dev, r.len * 4, "size"));
    GS_TRY(check_component_plane(info_out, g->buf->dev, sizeof(gs_components_info), "info"));
    if (!r.len && !info_out) return GS_OK;
    GS_TRY(use_device(r.dev));
    hipStream_t st = stream_of(r.dev, s);
    if (!r.len) {      // no kernel; the info of a graph without points
        GS_HIP(hipMemsetAsync(info_out->ptr, 0, 12, st));
        GS_HIP(hipMemsetAsync((char *)info_out->ptr + 12, 0xff, 4, st));
        return GS_OK;
    }
    // the event on every path: an enqueue that failed half-way has still left kernels on the scratch
    const gs_status rc = components_enqueue(g, st, among, mt, radius, labels_out ? (uint32_t *)labels_out->ptr : nullptr,
                                            sizes_out ? (uint32_t *)sizes_out->ptr : nullptr,
                                            info_out ? (uint32_t *)info_out->ptr : nullptr, nullptr, nullptr);
    const gs_status ev = neighbor_scratch_release(g, st);
    return rc != GS_OK ? rc : ev;
}

// sel = sel op {i : the plane's word of i is not 0 and lo <= it <= hi}, the plane made by components_enqueue; seeds: see there
static gs_status select_by_component(gs_selection *sel, gs_stream *s, gs_gaussians_buffer *g, const gs_selection *among,
                                     const gs_model_transform_pod *mt, float radius, const gs_selection *seeds, bool connected,
                                     uint32_t lo, uint32_t hi, gs_select_op op) {
    if (!sel || !g || (connected && !seeds)) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    GS_TRY(check_select_op(op));
    GS_TRY(check_neighbor_radius(radius));
    if (g->buf->dev != sel->dev) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "objects belong to different devices");
    GS_TRY(check_buffer_selection(g, s, among));
    if (connected) GS_TRY(check_buffer_selection(g, s, seeds));
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
    if (lo > hi) {      // sel = sel op {}
        sel->generation = next_object_id();
        sel_range_enqueue(sel, st, 0u, 0u, op);
        GS_HIP(hipGetLastError());
        return GS_OK;
    }
    uint32_t *plane = nullptr;
    gs_status rc = components_enqueue(g, st, among, mt, radius, nullptr, nullptr, nullptr, connected ? seeds->bits() : nullptr,
                                      &plane);
    if (rc == GS_OK) {      // only now does `sel` change; the seeds (which may be `sel`) were read by an earlier launch
        sel->generation = next_object_id();
        hipLaunchKernelGGL(gs::k_cc_select, dim3((n + 255u) / 256u), dim3(256), 0, st, (const uint32_t *)plane, n, lo, hi, sel->bits(),
                           (uint32_t)op);
        if (hipGetLastError() != hipSuccess) rc = gs_fail(GS_ERR_HIP, 0, 0, 0, "k_cc_select could not be launched");
    }
    // the event on every path: an enqueue that failed half-way has still left kernels on the scratch
    const gs_status ev = neighbor_scratch_release(g, st);
    return rc != GS_OK ? rc : ev;
}

extern "C" gs_status gs_select_components(gs_selection *sel, gs_stream *s, gs_gaussians_buffer *g, const gs_selection *among,
                                          const gs_model_transform_pod *mt, float radius, uint32_t min_size, uint32_t max_size,
                                          gs_select_op op) {
    return select_by_component(sel, s, g, among, mt, radius, nullptr, false, min_size, max_size, op);
}

extern "C" gs_status gs_select_connected(gs_selection *sel, gs_stream *s, gs_gaussians_buffer *g, const gs_selection *among,
                                         const gs_model_transform_pod *mt, float radius, const gs_selection *seeds, gs_select_op op) {
    return select_by_component(sel, s, g, among, mt, radius, seeds, true, 1u, 1u, op);
}
