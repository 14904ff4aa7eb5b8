// gs_simplify.hip — merge the Gaussians of each grid cell into one.  Kernels: gs_simplify_kernels.h; the
// grid, the sort and the scratch are the front of gs_neighbors.hip, the scan is the render unit's (gs_host.h).
#include "gs_host.h"

#include "gs_simplify_kernels.h"

using namespace gsh;

// ------------------------------------------------------------------------------------------------
// simplify
// ------------------------------------------------------------------------------------------------

// one merge kernel per pair of SH configs, one long-run kernel per destination SH config; the cov configs are kernel arguments
typedef void (*merge_fn)(const uint4 *, int, int, const uint64_t *, const uint32_t *, uint32_t, const float *, float, const uint32_t *,
                         uint32_t, uint32_t *, uint32_t *, uint4 *, uint32_t *, uint32_t);
#define GS_SH_ROW(s) {gs::k_sm_merge<s, 0>, gs::k_sm_merge<s, 1>, gs::k_sm_merge<s, 2>, gs::k_sm_merge<s, 3>}
static merge_fn k_tbl_merge[4][4] = {GS_SH_ROW(0), GS_SH_ROW(1), GS_SH_ROW(2), GS_SH_ROW(3)};
#undef GS_SH_ROW
typedef void (*long_fn)(const uint32_t *, uint32_t, int, const uint64_t *, const float *, float, uint32_t, uint32_t *, uint4 *, uint32_t);
static long_fn k_tbl_long[4] = {gs::k_sm_long<0>, gs::k_sm_long<1>, gs::k_sm_long<2>, gs::k_sm_long<3>};

static size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// Behind the shared front on `st`: the cells are counted, K comes to the host (the one round trip of the call), the result
// is allocated and both passes of the merge are enqueued and awaited.  n > 0, arguments checked.  *out stays null on failure.
static gs_status simplify_run(gs_gaussians_buffer *src, hipStream_t st, const gs_selection *among, float cell_size, int dsh, int dcov,
                              uint32_t *cell_of, gs_gaussians_buffer **out, uint64_t *count_out) {
    gs_device *dev = src->buf->dev;
    const uint32_t n = (uint32_t)gs_gaussians_buffer_len(src), nblocks = (n + 255u) / 256u, nwaves = (n + 63u) / 64u;
    // [cells per block, scanned in place][K][redo per cell][2 partials per wave of slots]
    const size_t b_counts = align256((size_t)nblocks * 4), b_redo = align256((size_t)n * 4);
    const size_t b_part = (size_t)nwaves * 2 * gs::SM_PART_WORDS * 4;
    NeighborGrid q;
    GS_TRY(neighbor_grid_enqueue(src, st, among, nullptr, cell_size, b_counts + 256 + b_redo + b_part, q));
    char *extra = (char *)q.extra;
    uint32_t *counts = (uint32_t *)extra, *total_dev = (uint32_t *)(extra + b_counts), *redo = (uint32_t *)(extra + b_counts + 256),
             *part = (uint32_t *)(extra + b_counts + 256 + b_redo);
    hipLaunchKernelGGL(gs::k_sm_count, dim3(nblocks), dim3(256), 0, st, q.keys, n, counts);
    scan_chunks_enqueue(st, counts, counts, total_dev, nblocks);
    hipError_t e = hipGetLastError();
    uint32_t K = 0;
    if (e == hipSuccess) e = fetch(st, &K, total_dev, 4);
    if (e != hipSuccess) return gs_fail(GS_ERR_HIP, (uint64_t)e, 0, 0, "cell count failed: %s", hipGetErrorString(e));
    if (K > n) return gs_fail(GS_ERR_HIP, K, n, 0, "cell count returned %u cells of %u Gaussians", K, n);
    gs_gaussians_buffer *dst = nullptr;
    if (K) {
        GS_TRY(gaussians_buffer_create_unfilled(dev, dsh, dcov, K, &dst));
        for (uint32_t unit = 0; unit < 2u; unit++) {
            hipLaunchKernelGGL(k_tbl_merge[src->sh][dsh], dim3(nblocks), dim3(256), 0, st, (const uint4 *)src->buf->ptr, src->cov, dcov,
                               q.keys, q.vals, n, q.bbox, cell_size, (const uint32_t *)counts, unit, redo, part, (uint4 *)dst->buf->ptr,
                               cell_of, K);
            hipLaunchKernelGGL(k_tbl_long[dsh], dim3((nwaves + 3u) / 4u), dim3(256), 0, st, (const uint32_t *)part, n, dcov, q.keys,
                               q.bbox, cell_size, unit, redo, (uint4 *)dst->buf->ptr, K);
        }
        e = hipGetLastError();
    } else {
        GS_TRY(gs_gaussians_buffer_create(dev, (gs_sh_config)dsh, (gs_cov3d_config)dcov, nullptr, 0, &dst));
        if (cell_of) e = hipMemsetAsync(cell_of, 0xff, (size_t)n * 4, st);      // no Gaussian is a point
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);      // the call is blocking: the result is complete when it returns
    if (e != hipSuccess) {
        gs_gaussians_buffer_destroy(dst);
        return gs_fail(GS_ERR_HIP, (uint64_t)e, 0, 0, "simplification failed: %s", hipGetErrorString(e));
    }
    dst->spatial = src->spatial;
    *out = dst;
    if (count_out) *count_out = K;
    return GS_OK;
}

extern "C" gs_status gs_gaussians_buffer_create_simplified(gs_gaussians_buffer *src, gs_stream *s, const gs_selection *among,
                                                           float cell_size, gs_sh_config dst_sh, gs_cov3d_config dst_cov,
                                                           gs_buffer *cell_of_out, gs_gaussians_buffer **out, uint64_t *count_out) {
    if (out) *out = nullptr;
    if (count_out) *count_out = 0;
    if (!src || !out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    if (!valid_cfg(dst_sh, dst_cov)) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "unknown layout config");
    GS_TRY(check_neighbor_radius(cell_size));
    RecordsAccess r;
    GS_TRY(records_check(src, s, among, 0, r));
    if (cell_of_out) {
        if (cell_of_out->dev != r.dev) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "objects belong to different devices");
        if (cell_of_out->bytes < r.len * 4)
            return gs_fail(GS_ERR_INVALID_ARGUMENT, cell_of_out->bytes, r.len * 4, 0, "the cell plane has %zu bytes, %zu Gaussians need %zu",
                           cell_of_out->bytes, r.len, r.len * 4);
    }
    GS_TRY(use_device(r.dev));
    if (!r.len) {      // no kernel, no scratch
        gs_gaussians_buffer *dst = nullptr;
        GS_TRY(gs_gaussians_buffer_create(r.dev, dst_sh, dst_cov, nullptr, 0, &dst));
        dst->spatial = src->spatial;
        *out = dst;
        return GS_OK;
    }
    hipStream_t st = stream_of(r.dev, s);
    // the event on every path: an enqueue that failed half-way has still left kernels on the scratch
    const gs_status rc = simplify_run(src, st, among, cell_size, dst_sh, dst_cov, cell_of_out ? (uint32_t *)cell_of_out->ptr : nullptr, out,
                                      count_out);
    const gs_status ev = neighbor_scratch_release(src, st);
    if (rc == GS_OK && ev != GS_OK) {
        gs_gaussians_buffer_destroy(*out);
        *out = nullptr;
        if (count_out) *count_out = 0;
    }
    return rc != GS_OK ? rc : ev;
}
