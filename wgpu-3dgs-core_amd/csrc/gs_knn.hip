// gs_knn.hip — the k nearest neighbours of every point, select by them, their summary.  Kernels:
// gs_knn_kernels.h; the grid, the sort and the scratch are the front of gs_neighbors.hip.
#include "gs_host.h"

#include "gs_knn_kernels.h"

using namespace gsh;

// ------------------------------------------------------------------------------------------------
// k nearest neighbours
// ------------------------------------------------------------------------------------------------

// one traversal kernel per k: the row of a lane is K registers pairs, indexed by constants only
typedef void (*knn_fn)(const uint64_t *, const uint32_t *, const float *, const float *, const float *, uint32_t, float, const uint32_t *,
                       uint32_t *, uint32_t *);
static knn_fn k_tbl_knn[gs::KNN_MAX_K] = {gs::k_nb_knn<1>,  gs::k_nb_knn<2>,  gs::k_nb_knn<3>,  gs::k_nb_knn<4>,
                                          gs::k_nb_knn<5>,  gs::k_nb_knn<6>,  gs::k_nb_knn<7>,  gs::k_nb_knn<8>,
                                          gs::k_nb_knn<9>,  gs::k_nb_knn<10>, gs::k_nb_knn<11>, gs::k_nb_knn<12>,
                                          gs::k_nb_knn<13>, gs::k_nb_knn<14>, gs::k_nb_knn<15>, gs::k_nb_knn<16>};

static_assert(GS_KNN_MAX_K == gs::KNN_MAX_K && GS_KNN_NONE == gs::KNN_NONE, "the header's constants are the kernels'");
static_assert((int)GS_KNN_KTH_DIST2 == (int)gs::KNN_KTH_DIST2 && (int)GS_KNN_MEAN_DIST == (int)gs::KNN_MEAN_DIST, "... and its statistics");

static gs_status check_knn_k(uint32_t k) {
    if (k < 1u || k > gs::KNN_MAX_K) return gs_fail(GS_ERR_INVALID_ARGUMENT, k, gs::KNN_MAX_K, 0, "k must be 1 to %u, not %u", (unsigned)gs::KNN_MAX_K, (unsigned)k);
    return GS_OK;
}
static gs_status check_knn_kind(uint32_t kind) {
    if (kind > (uint32_t)GS_KNN_MEAN_DIST) return gs_fail(GS_ERR_INVALID_ARGUMENT, kind, 0, 0, "unknown k-NN statistic %u", (unsigned)kind);
    return GS_OK;
}
// a plane of n rows of k words on `dev`
static gs_status check_knn_plane(const gs_buffer *plane, const gs_device *dev, size_t n, uint32_t k, const char *what) {
    if (plane->dev != dev) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "objects belong to different devices");
    const size_t need = n * 4 * k;
    if (plane->bytes < need)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, plane->bytes, need, 0, "the %s plane has %zu bytes, %zu rows of %u need %zu", what, plane->bytes, n,
                       (unsigned)k, need);
    return GS_OK;
}

extern "C" gs_status gs_gaussians_buffer_knn(gs_gaussians_buffer *g, gs_stream *s, const gs_selection *among, const gs_selection *queries,
                                             const gs_model_transform_pod *mt, uint32_t k, float radius, gs_buffer *dist2_out,
                                             gs_buffer *index_out) {
    if (!g || !dist2_out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    GS_TRY(check_neighbor_radius(radius));
    GS_TRY(check_knn_k(k));
    RecordsAccess r;
    GS_TRY(records_check(g, s, among, 0, r));
    GS_TRY(check_buffer_selection(g, s, queries));
    GS_TRY(check_knn_plane(dist2_out, r.dev, r.len, k, "distance"));
    if (index_out) GS_TRY(check_knn_plane(index_out, r.dev, r.len, k, "index"));
    if (!r.len) return GS_OK;
    GS_TRY(use_device(r.dev));
    hipStream_t st = stream_of(r.dev, s);
    NeighborGrid q;
    gs_status rc = neighbor_grid_enqueue(g, st, among, mt, radius, 0, q);
    if (rc == GS_OK) {
        hipLaunchKernelGGL(k_tbl_knn[k - 1u], dim3(q.nblocks), dim3(256), 0, st, q.keys, q.vals, q.sx, q.sy, q.sz, q.n, radius * radius,
                           queries ? (const uint32_t *)queries->bits() : nullptr, (uint32_t *)dist2_out->ptr,
                           index_out ? (uint32_t *)index_out->ptr : nullptr);
        if (hipGetLastError() != hipSuccess) rc = gs_fail(GS_ERR_HIP, 0, 0, 0, "k_nb_knn could not be launched");
    }
    // the event on every path: an enqueue that failed half-way has still left kernels on the scratch
    const gs_status ev = neighbor_scratch_release(g, st);
    return rc != GS_OK ? rc : ev;
}

extern "C" gs_status gs_select_knn(gs_selection *sel, gs_stream *s, const gs_buffer *plane, uint32_t k, uint32_t kind, float lo, float hi,
                                   gs_select_op op) {
    if (!sel || !plane) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    GS_TRY(check_select_op(op));
    GS_TRY(check_knn_k(k));
    GS_TRY(check_knn_kind(kind));
    if (lo != lo || hi != hi) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "a bound is NaN");
    if (s && s->dev != sel->dev) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "objects belong to different devices");
    GS_TRY(check_len32(sel->n));
    GS_TRY(check_knn_plane(plane, sel->dev, sel->n, k, "distance"));
    GS_TRY(use_device(sel->dev));
    hipStream_t st = stream_of(sel->dev, s);
    sel->generation = next_object_id();
    if (!sel->n) return GS_OK;
    const uint32_t n = (uint32_t)sel->n;
    if (lo > hi)      // sel = sel op {}
        sel_range_enqueue(sel, st, 0u, 0u, op);
    else
        hipLaunchKernelGGL(gs::k_knn_select, dim3((n + 255u) / 256u), dim3(256), 0, st, (const float *)plane->ptr, n, k, kind, lo, hi, sel->bits(),
                           (uint32_t)op);
    GS_HIP(hipGetLastError());
    return GS_OK;
}

extern "C" gs_status gs_knn_summary(gs_stream *s, const gs_buffer *plane, uint64_t n, uint32_t k, uint32_t kind, gs_knn_summary_result *out) {
    if (!plane || !out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    GS_TRY(check_knn_k(k));
    GS_TRY(check_knn_kind(kind));
    if (s && s->dev != plane->dev) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "objects belong to different devices");
    GS_TRY(check_len32((size_t)n));
    GS_TRY(check_knn_plane(plane, plane->dev, (size_t)n, k, "distance"));
    static_assert(sizeof(gs::KnnSummaryOut) == sizeof(gs_knn_summary_result), "the device result is a gs_knn_summary_result");
    gs_knn_summary_result res;
    std::memset(&res, 0, sizeof(res));
    res.min = INFINITY;
    res.max = -INFINITY;
    if (n) {
        gs_device *dev = plane->dev;
        GS_TRY(use_device(dev));
        hipStream_t st = stream_of(dev, s);
        const uint32_t rows = (uint32_t)n, nblocks = (rows + 255u) / 256u;
        // [the result, 256 bytes][the sums: 2 x nblocks doubles][the integer fields: 4 x nblocks words]; the call is blocking, so
        // the array is the call's own and is awaited before it goes
        const size_t d_bytes = (size_t)gs::KNN_D_FIELDS * nblocks * 8, u_bytes = (size_t)gs::KNN_U_FIELDS * nblocks * 4;
        DevMem scratch;
        GS_TRY(scratch.alloc(256 + d_bytes + u_bytes, 256 + d_bytes + u_bytes, "k-NN summary scratch allocation"));
        gs::KnnSummaryOut *dout = (gs::KnnSummaryOut *)scratch.ptr;
        double *part_d = (double *)((char *)scratch.ptr + 256);
        uint32_t *part_u = (uint32_t *)((char *)scratch.ptr + 256 + d_bytes);
        hipLaunchKernelGGL(gs::k_knn_summary_partial, dim3(nblocks), dim3(256), 0, st, (const float *)plane->ptr, rows, k, kind, part_u, part_d,
                           nblocks);
        hipLaunchKernelGGL(gs::k_knn_summary_finish, dim3(1), dim3(256), 0, st, (const uint32_t *)part_u, (const double *)part_d, nblocks, dout);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&res, dout, sizeof(res), hipMemcpyDeviceToHost, st);
        const hipError_t w = hipStreamSynchronize(st);      // on every path: the kernels have left the array
        if (e == hipSuccess) e = w;
        if (e != hipSuccess) return gs_fail(GS_ERR_DOWNLOAD, (uint64_t)e, 0, 0, "download failed: %s", hipGetErrorString(e));
    }
    *out = res;
    return GS_OK;
}
