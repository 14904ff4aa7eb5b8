// gs_align.hip — nearest neighbours between two buffers, the correspondence sums of their pairs and the closed-form rigid
// fit.  Kernels: gs_align_kernels.h; the target's grid, the sort and the scratch are the front of
// gs_neighbors.hip; the host arithmetic of the fit: gs_align_fit.h.
#include "gs_host.h"

#include "gs_align_fit.h"
#include "gs_align_kernels.h"

using namespace gsh;

// ------------------------------------------------------------------------------------------------
// k nearest neighbours between two buffers
// ------------------------------------------------------------------------------------------------

// one traversal kernel per k, as gs_knn.hip has them
typedef void (*knn_between_fn)(const uint64_t *, const uint32_t *, const float *, const float *, const float *, uint32_t, const uint64_t *,
                               const uint32_t *, const float *, const float *, const float *, uint32_t, float, uint32_t *, uint32_t *);
static knn_between_fn k_tbl_knn_between[gs::AL_MAX_K] = {
    gs::k_nb_knn_between<1>,  gs::k_nb_knn_between<2>,  gs::k_nb_knn_between<3>,  gs::k_nb_knn_between<4>,
    gs::k_nb_knn_between<5>,  gs::k_nb_knn_between<6>,  gs::k_nb_knn_between<7>,  gs::k_nb_knn_between<8>,
    gs::k_nb_knn_between<9>,  gs::k_nb_knn_between<10>, gs::k_nb_knn_between<11>, gs::k_nb_knn_between<12>,
    gs::k_nb_knn_between<13>, gs::k_nb_knn_between<14>, gs::k_nb_knn_between<15>, gs::k_nb_knn_between<16>};

static_assert(GS_KNN_MAX_K == gs::AL_MAX_K && GS_KNN_NONE == gs::AL_NONE, "the header's constants are the kernels'");
static_assert(sizeof(gs::PairSumsOut) == sizeof(gs_pair_sums) && sizeof(gs_pair_sums) == 152, "the device result is a gs_pair_sums");

static gs_status check_k(uint32_t k) {
    if (k < 1u || k > gs::AL_MAX_K) return gs_fail(GS_ERR_INVALID_ARGUMENT, k, gs::AL_MAX_K, 0, "k must be 1 to %u, not %u", (unsigned)gs::AL_MAX_K, (unsigned)k);
    return GS_OK;
}
// a plane of n rows of k words on `dev`
static gs_status check_plane(const gs_buffer *plane, const gs_device *dev, size_t n, uint32_t k, const char *what) {
    if (plane->dev != dev) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "objects belong to different devices");
    const size_t need = n * 4 * k;
    if (plane->bytes < need)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, plane->bytes, need, 0, "the %s plane has %zu bytes, %zu rows of %u need %zu", what, plane->bytes, n,
                       (unsigned)k, need);
    return GS_OK;
}
static void shape_of(const gs_model_transform_pod *mt, float M[16]) {
    gs_model_transform_pod def;
    if (!mt) {
        gs_model_transform_pod_default(&def);
        mt = &def;
    }
    gs::ModelTransform m;
    std::memcpy(&m, mt, sizeof(m));
    gs::model_transform_mat(m, M);
}

// The query side, on `st` behind the target's grid: the keys of the queries in that grid, sorted in the query buffer's
// scratch, their positions gathered; then the traversal.  nq > 0, arguments checked, the scratch reserved.
static gs_status knn_between_enqueue(gs_gaussians_buffer *qb, hipStream_t st, const gs_selection *queries, const gs_model_transform_pod *qmt,
                                     const NeighborGrid &t, float radius, uint32_t k, uint32_t *dist2, uint32_t *index) {
    gs_device *dev = qb->buf->dev;
    const uint32_t n = (uint32_t)gs_gaussians_buffer_len(qb), pod_words = (uint32_t)(pod_stride(qb) / 4), nblocks = (n + 255u) / 256u;
    // [keys 0][vals 0][keys 1][vals 1], the layout of neighbor_grid_enqueue: the sorted positions take the pair the sort did
    // not leave its result in
    const size_t a8 = ((size_t)n * 8 + 255) & ~(size_t)255, a4 = ((size_t)n * 4 + 255) & ~(size_t)255;
    char *base = (char *)qb->nb_scratch.ptr;
    void *k2[2] = {base, base + a8 + a4};
    void *v2[2] = {base + a8, base + 2 * a8 + a4};
    // an edit enqueued on another stream still writes the records; a call on another stream still reads the scratch
    GS_TRY(wait_for_edits(qb, st));
    if (qb->nb_done && st != qb->nb_stream) GS_HIP(hipStreamWaitEvent(st, qb->nb_done, 0));
    gs::SelectShape sh{};
    shape_of(qmt, sh.M);
    const uint32_t *aos = (const uint32_t *)qb->buf->ptr;
    hipLaunchKernelGGL(gs::k_al_query_keys, dim3(nblocks), dim3(256), 0, st, aos, pod_words, n, queries ? (const uint32_t *)queries->bits() : nullptr,
                       sh, t.bbox, radius, (uint64_t *)k2[0], (uint32_t *)v2[0]);
    GS_HIP(hipGetLastError());
    int side = 0;
    uint32_t passes = 0;
    GS_TRY(sort_pairs_device<uint64_t>(dev, k2, v2, qb->nb_ghist, qb->nb_digit_totals, n, 64, st, side, passes));
    const uint64_t *skeys = (const uint64_t *)k2[side];
    const uint32_t *svals = (const uint32_t *)v2[side];
    float *sx = (float *)k2[side ^ 1], *sy = sx + n, *sz = sy + n;      // 12 n bytes <= a8 + a4, the pair is contiguous
    hipLaunchKernelGGL(gs::k_al_query_gather, dim3(nblocks), dim3(256), 0, st, aos, pod_words, n, sh, skeys, svals, sx, sy, sz);
    hipLaunchKernelGGL(k_tbl_knn_between[k - 1u], dim3(nblocks), dim3(256), 0, st, t.keys, t.vals, t.sx, t.sy, t.sz, t.n, skeys, svals,
                       (const float *)sx, (const float *)sy, (const float *)sz, n, radius * radius, dist2, index);
    GS_HIP(hipGetLastError());
    return GS_OK;
}

extern "C" gs_status gs_gaussians_buffer_knn_between(gs_gaussians_buffer *qb, gs_gaussians_buffer *target, gs_stream *s,
                                                     const gs_selection *queries, const gs_selection *among,
                                                     const gs_model_transform_pod *qmt, const gs_model_transform_pod *tmt, uint32_t k,
                                                     float radius, gs_buffer *dist2_out, gs_buffer *index_out) {
    if (!qb || !target || !dist2_out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    if (qb == target) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "the two buffers are one: that is gs_gaussians_buffer_knn");
    if (qb->buf->dev != target->buf->dev) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "objects belong to different devices");
    GS_TRY(check_neighbor_radius(radius));
    GS_TRY(check_k(k));
    RecordsAccess rq, rt;
    GS_TRY(records_check(qb, s, queries, 0, rq));
    GS_TRY(records_check(target, s, among, 0, rt));
    GS_TRY(check_plane(dist2_out, rq.dev, rq.len, k, "distance"));
    if (index_out) GS_TRY(check_plane(index_out, rq.dev, rq.len, k, "index"));
    if (!rq.len) return GS_OK;
    GS_TRY(use_device(rq.dev));
    hipStream_t st = stream_of(rq.dev, s);
    // the query scratch before anything is enqueued: growing it frees the old array
    const size_t a8 = ((size_t)rq.n * 8 + 255) & ~(size_t)255, a4 = ((size_t)rq.n * 4 + 255) & ~(size_t)255;
    GS_TRY(dev_reserve(qb->nb_scratch, 2 * (a8 + a4)));
    NeighborGrid t;      // a target of length 0: no grid, no box, and every query point is far from it
    gs_status rc = rt.len ? neighbor_grid_enqueue(target, st, among, tmt, radius, 0, t) : GS_OK;
    if (rc == GS_OK)
        rc = knn_between_enqueue(qb, st, queries, qmt, t, radius, k, (uint32_t *)dist2_out->ptr, index_out ? (uint32_t *)index_out->ptr : nullptr);
    // the events on every path: an enqueue that failed half-way has still left kernels on the scratch of either buffer
    const gs_status ev_t = rt.len ? neighbor_scratch_release(target, st) : GS_OK;
    const gs_status ev_q = neighbor_scratch_release(qb, st);
    return rc != GS_OK ? rc : ev_t != GS_OK ? ev_t : ev_q;
}

// ------------------------------------------------------------------------------------------------
// the sums over the pairs of an index plane
// ------------------------------------------------------------------------------------------------

extern "C" gs_status gs_gaussians_buffer_pair_sums(gs_gaussians_buffer *qb, gs_gaussians_buffer *target, gs_stream *s,
                                                   const gs_selection *queries, const gs_model_transform_pod *qmt,
                                                   const gs_model_transform_pod *tmt, const gs_buffer *index_plane, uint32_t k,
                                                   gs_pair_sums *out) {
    if (!qb || !target || !index_plane || !out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    if (qb->buf->dev != target->buf->dev) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "objects belong to different devices");
    GS_TRY(check_k(k));
    RecordsAccess rq, rt;
    GS_TRY(records_check(qb, s, queries, 0, rq));
    GS_TRY(records_check(target, s, nullptr, 0, rt));
    GS_TRY(check_plane(index_plane, rq.dev, rq.len, k, "index"));
    gs_pair_sums res;
    std::memset(&res, 0, sizeof(res));
    if (rq.len) {
        GS_TRY(use_device(rq.dev));
        hipStream_t st = stream_of(rq.dev, s);
        const uint32_t nblocks = (rq.n + 255u) / 256u;
        // [the result, 256 bytes][the sums: 18 x nblocks doubles][the counts: nblocks words]; the call is blocking, so the
        // array is the call's own and is awaited before it goes
        const size_t d_bytes = (size_t)gs::AL_D_FIELDS * nblocks * 8, u_bytes = (size_t)nblocks * 4;
        DevMem scratch;
        GS_TRY(scratch.alloc(256 + d_bytes + u_bytes, 256 + d_bytes + u_bytes, "pair sums scratch allocation"));
        // an edit enqueued on another stream still writes the records of either buffer
        GS_TRY(wait_for_edits(qb, st));
        GS_TRY(wait_for_edits(target, st));
        gs::PairSumsOut *dout = (gs::PairSumsOut *)scratch.ptr;
        double *part_d = (double *)((char *)scratch.ptr + 256);
        uint32_t *part_u = (uint32_t *)((char *)scratch.ptr + 256 + d_bytes);
        gs::PairShapes sh;
        shape_of(qmt, sh.Mq);
        shape_of(tmt, sh.Mt);
        hipLaunchKernelGGL(gs::k_al_pair_partial, dim3(nblocks), dim3(256), 0, st, (const uint32_t *)qb->buf->ptr, (uint32_t)(pod_stride(qb) / 4),
                           rq.n, rq.words, (const uint32_t *)target->buf->ptr, (uint32_t)(pod_stride(target) / 4), rt.n, sh,
                           (const uint32_t *)index_plane->ptr, k, part_u, part_d, nblocks);
        hipLaunchKernelGGL(gs::k_al_pair_finish, dim3(1), dim3(256), 0, st, (const uint32_t *)part_u, (const double *)part_d, nblocks, dout);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&res, dout, sizeof(res), hipMemcpyDeviceToHost, st);
        const hipError_t w = hipStreamSynchronize(st);      // on every path: the kernels have left the array
        if (e == hipSuccess) e = w;
        if (e != hipSuccess) return gs_fail(GS_ERR_DOWNLOAD, (uint64_t)e, 0, 0, "download failed: %s", hipGetErrorString(e));
    }
    *out = res;
    return GS_OK;
}

// ------------------------------------------------------------------------------------------------
// the closed-form fit and the composition of two transforms: host, binary64, no device
// ------------------------------------------------------------------------------------------------

extern "C" gs_status gs_rigid_fit(const gs_pair_sums *sums, int32_t with_scale, gs_model_transform_pod *delta_out, double *rms_out) {
    if (!sums || !delta_out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    const char *why = gsfit::rigid_fit(sums, with_scale, delta_out, rms_out);
    if (why) return gs_fail(GS_ERR_INVALID_ARGUMENT, sums->pairs, 0, 0, "%s", why);
    return GS_OK;
}

extern "C" void gs_model_transform_compose(const gs_model_transform_pod *delta, const gs_model_transform_pod *m, gs_model_transform_pod *out) {
    if (!delta || !m || !out) return;
    gsfit::compose(delta, m, out);
}
