// gs_edit.hip — the write side of the device editor: SH rotation matrices, edits of the selected Gaussians, extraction
// (DESIGN.md §3.8), snapshots and restore (§3.9; the concatenation's body is gs_relayout.hip's).  Kernels: gs_edit_kernels.h.
#include "gs_host.h"

#include "gs_edit_kernels.h"

using namespace gsh;

// ------------------------------------------------------------------------------------------------
// edits of the selected Gaussians, extraction
// ------------------------------------------------------------------------------------------------

// the basis of DESIGN.md §3.2 for one band (l = 1, 2, 3: 3, 5, 7 functions), in double
static void sh_band_basis(int l, const double d[3], double *Y) {
    const double x = d[0], y = d[1], z = d[2], xx = x * x, yy = y * y, zz = z * z;
    if (l == 1) {
        const double C1 = 0.4886025119029199;
        Y[0] = -C1 * y;
        Y[1] = C1 * z;
        Y[2] = -C1 * x;
    } else if (l == 2) {
        Y[0] = 1.0925484305920792 * x * y;
        Y[1] = -1.0925484305920792 * y * z;
        Y[2] = 0.31539156525252005 * (2.0 * zz - xx - yy);
        Y[3] = -1.0925484305920792 * x * z;
        Y[4] = 0.5462742152960396 * (xx - yy);
    } else {
        Y[0] = -0.5900435899266435 * y * (3.0 * xx - yy);
        Y[1] = 2.890611442640554 * x * y * z;
        Y[2] = -0.4570457994644658 * y * (4.0 * zz - xx - yy);
        Y[3] = 0.3731763325901154 * z * (2.0 * zz - 3.0 * xx - 3.0 * yy);
        Y[4] = -0.4570457994644658 * x * (4.0 * zz - xx - yy);
        Y[5] = 1.445305721320277 * z * (xx - yy);
        Y[6] = -0.5900435899266435 * x * (xx - 3.0 * yy);
    }
}

// D of one band from its defining property: B D = B' over sample directions d_i, B[i][k] = Y_k(d_i),
// B'[i][k] = Y_k(R^T d_i); solved as the normal equations (B^T B) D = B^T B' by Gaussian elimination with partial
// pivoting.  The band's functions span a rotation-invariant space, so the system is consistent and D is exact up to
// double rounding.
static bool sh_band_rotation(int l, const double R[3][3], float *out) {
    const int nb = 2 * l + 1, NS = 64;
    double N[7][14] = {};      // [B^T B | B^T B']
    for (int i = 0; i < NS; i++) {
        // Fibonacci sphere: well spread, no symmetry that a band could hide in
        const double z = 1.0 - (2.0 * i + 1.0) / NS, r = std::sqrt(1.0 - z * z), phi = i * 2.399963229728653;
        const double d[3] = {r * std::cos(phi), r * std::sin(phi), z};
        double dr[3];
        for (int a = 0; a < 3; a++) dr[a] = (R[0][a] * d[0] + R[1][a] * d[1]) + R[2][a] * d[2];     // R^T d
        double Y[7], Yr[7];
        sh_band_basis(l, d, Y);
        sh_band_basis(l, dr, Yr);
        for (int k = 0; k < nb; k++)
            for (int j = 0; j < nb; j++) {
                N[k][j] += Y[k] * Y[j];
                N[k][nb + j] += Y[k] * Yr[j];
            }
    }
    for (int c = 0; c < nb; c++) {
        int p = c;
        for (int r = c + 1; r < nb; r++)
            if (std::fabs(N[r][c]) > std::fabs(N[p][c])) p = r;
        if (!(std::fabs(N[p][c]) > 1e-12)) return false;
        if (p != c)
            for (int j = 0; j < 2 * nb; j++) std::swap(N[p][j], N[c][j]);
        for (int r = 0; r < nb; r++) {
            if (r == c) continue;
            const double f = N[r][c] / N[c][c];
            for (int j = c; j < 2 * nb; j++) N[r][j] -= f * N[c][j];
        }
    }
    // the entries are polynomials in R of magnitude <= 1; what the solve leaves below 1e-14 is its own rounding noise
    // (the identity must give the identity)
    for (int k = 0; k < nb; k++)
        for (int j = 0; j < nb; j++) {
            const double v = N[k][nb + j] / N[k][k];
            out[k * nb + j] = std::fabs(v) < 1e-14 ? 0.0f : (float)v;
        }
    return true;
}

extern "C" gs_status gs_sh_rotation_matrices(const float rot_xyzw[4], float d1[9], float d2[25], float d3[49]) {
    if (!rot_xyzw || !d1 || !d2 || !d3) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    double q[4], len2 = 0.0;
    for (int k = 0; k < 4; k++) {
        q[k] = (double)rot_xyzw[k];
        len2 += q[k] * q[k];
    }
    if (!std::isfinite(len2) || !(len2 > 0.0)) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "the rotation must be finite and nonzero");
    const double inv = 1.0 / std::sqrt(len2);
    const double x = q[0] * inv, y = q[1] * inv, z = q[2] * inv, w = q[3] * inv;
    const double R[3][3] = {{1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)},
                            {2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)},
                            {2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)}};
    if (!sh_band_rotation(1, R, d1) || !sh_band_rotation(2, R, d2) || !sh_band_rotation(3, R, d3))
        return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "the rotation is degenerate");
    return GS_OK;
}

typedef void (*edit_fn)(uint4 *, uint32_t, const uint32_t *, gs::EditArgs);
static edit_fn k_tbl_edit[4][3] = GS_CFG_TABLE(gs::k_edit);

extern "C" gs_status gs_gaussians_buffer_edit(gs_gaussians_buffer *g, gs_stream *s, const gs_selection *sel, const gs_edit *e) {
    if (!g || !e) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    const uint32_t known = GS_EDIT_TRANSFORM | GS_EDIT_ROTATE_SH | GS_EDIT_COLOR | GS_EDIT_OPACITY;
    if (e->flags & ~known) return gs_fail(GS_ERR_INVALID_ARGUMENT, e->flags, 0, 0, "unknown gs_edit flags 0x%x", (unsigned)e->flags);
    for (uint32_t r : e->reserved)
        if (r) return gs_fail(GS_ERR_INVALID_ARGUMENT, r, 0, 0, "gs_edit.reserved must be 0");
    if ((e->flags & GS_EDIT_ROTATE_SH) && !(e->flags & GS_EDIT_TRANSFORM))
        return gs_fail(GS_ERR_INVALID_ARGUMENT, e->flags, 0, 0, "GS_EDIT_ROTATE_SH goes with GS_EDIT_TRANSFORM");
    gs::EditArgs a{};
    a.flags = e->flags;
    if (e->flags & GS_EDIT_TRANSFORM) {
        const gs_model_transform_pod &t = e->transform;
        if (!all_finite(t.pos, 3) || !all_finite(t.rot, 4) || !all_finite(t.scale, 3))
            return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "the transform of an edit must be finite");
        if (!(t.scale[0] > 0.0f) || t.scale[1] != t.scale[0] || t.scale[2] != t.scale[0])
            return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "the scale of an edit must be uniform and positive");
        gs::ModelTransform m;
        std::memcpy(&m, &t, sizeof(m));
        gs::model_transform_mat(m, a.M);
        gs::model_scale_rot_mat(m, a.A);
        std::memcpy(a.q, t.rot, sizeof(a.q));
        a.s = t.scale[0];
        if (e->flags & GS_EDIT_ROTATE_SH) GS_TRY(gs_sh_rotation_matrices(t.rot, a.D1, a.D2, a.D3));
    }
    if (e->flags & GS_EDIT_COLOR) {
        if (!all_finite(e->color, 12)) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "the colour matrix of an edit must be finite");
        std::memcpy(a.C, e->color, sizeof(a.C));
    }
    if (e->flags & GS_EDIT_OPACITY) {
        if (!all_finite(e->opacity, 2)) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "the opacity terms of an edit must be finite");
        std::memcpy(a.o, e->opacity, sizeof(a.o));
    }
    RecordsAccess r;
    GS_TRY(records_check(g, s, sel, 0, r));
    const size_t len = r.len;
    if (g->sh == GS_SH_NONE) a.flags &= ~(uint32_t)GS_EDIT_ROTATE_SH;
    if (!a.flags || !len) return GS_OK;
    GS_TRY(use_device(r.dev));
    hipStream_t st = stream_of(r.dev, s);
    // a mirror rebuild in flight on another stream still reads the records (the one wait of this call: it takes the
    // checks of records_access, not its wait for edits)
    if (g->mirror_ready && st != g->mirror_stream) GS_HIP(hipStreamWaitEvent(st, g->mirror_ready, 0));
    hipLaunchKernelGGL(k_tbl_edit[g->sh][g->cov], dim3((r.n + 255u) / 256u), dim3(256), 0, st, (uint4 *)g->buf->ptr, r.n, r.words, a);
    GS_HIP(hipGetLastError());
    GS_TRY(record_edit(g, st));
    // The host does not know which Gaussians the selection names: the whole mirror is stale.  A transform moves them,
    // so the next frame sorts the spatial order again, exactly as after an upload of the edited records; a colour /
    // opacity edit keeps every position, and with it the order (only the repack and the block bounds run again).
    if (a.flags & GS_EDIT_TRANSFORM) {
        g->mark_all();
    } else if (!(g->dirty_lo == 0 && g->dirty_hi >= len)) {
        g->dirty_lo = 0;
        g->dirty_hi = len;
        g->keep_order = true;
    }
    return GS_OK;
}

// A buffer of `len` > 0 records for a copy that writes every byte of it: allocated WITHOUT the zero fill of
// gs_buffer_create: that hipMemset runs on the null stream, which the copy's stream is not ordered behind, and would race
// with the copy.
gs_status gsh::gaussians_buffer_create_unfilled(gs_device *dev, int sh, int cov, size_t len, gs_gaussians_buffer **out) {
    DevMem p;
    const size_t bytes = len * (size_t)gs::pod_bytes(sh, cov);
    GS_TRY(p.alloc(bytes, bytes, "hipMalloc"));
    gs_buffer *b = make_buffer(dev, p.release(), bytes, true);
    gs_status rc = gs_gaussians_buffer_from_buffer(b, (gs_sh_config)sh, (gs_cov3d_config)cov, out);
    gs_buffer_release(b);
    return rc;
}

// The prelude of every extraction, on `st`: the selected (invert: the unselected) Gaussians of each 1024-block of a mask
// of n > 0 bits are counted into `offsets`, scanned there in place (k_scan_chunks reads a value before it writes its
// slot) and summed into *total_dev.  Only enqueued: gs_gaussians_buffer_create_concat fetches the totals of all its
// sources in one round trip.
void gsh::extract_scan_enqueue(hipStream_t st, const uint32_t *words, uint32_t n, uint32_t invert, uint32_t *offsets, uint32_t *total_dev) {
    const uint32_t nblocks = (n + gs::PLANAR_BLOCK - 1u) / gs::PLANAR_BLOCK;
    hipLaunchKernelGGL(gs::k_extract_block_counts, dim3((nblocks * 32u + 255u) / 256u), dim3(256), 0, st, words, n, invert, nblocks, offsets);
    scan_chunks_enqueue(st, offsets, offsets, total_dev, nblocks);
}

// ... and its total on the host, which sizing the destination needs: blocks on `st`
gs_status gsh::extract_scan(hipStream_t st, const uint32_t *words, uint32_t n, uint32_t invert, uint32_t *offsets, uint32_t *total_dev,
                              uint32_t *total) {
    extract_scan_enqueue(st, words, n, invert, offsets, total_dev);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = fetch(st, total, total_dev, 4);
    if (e != hipSuccess) return gs_fail(GS_ERR_HIP, (uint64_t)e, 0, 0, "selection scan failed: %s", hipGetErrorString(e));
    if (*total > n) return gs_fail(GS_ERR_HIP, *total, n, 0, "selection scan returned %u of %u Gaussians", *total, n);
    return GS_OK;
}

// what extraction, conversion and the exports start with: the prelude, the scan into an array of the call (freed with `x`,
// after whatever the caller enqueues on it has been awaited) and its total.  An empty buffer is scanned by nobody.
gs_status gsh::extract_begin(const gs_gaussians_buffer *g, gs_stream *s, const gs_selection *sel, int32_t invert, ExtractScan &x) {
    GS_TRY(records_access(g, s, sel, invert, x));
    if (!x.n) return GS_OK;
    GS_TRY(dev_reserve(x.scan, ((size_t)x.nblocks + 1) * 4));
    return extract_scan(x.st, x.words, x.n, x.inv, (uint32_t *)x.scan.ptr, (uint32_t *)x.scan.ptr + x.nblocks, &x.total);
}

// the `total` records the scan counted: src (n records of nc 16-byte chunks) -> dst, packed in index order
void gsh::extract_copy_enqueue(hipStream_t st, const void *src, void *dst, const uint32_t *words, uint32_t n, uint32_t invert,
                                 const uint32_t *offsets, uint32_t nc, uint32_t total) {
    hipLaunchKernelGGL(gs::k_extract_copy, dim3((n + 255u) / 256u), dim3(256), 0, st, (const uint4 *)src, (uint4 *)dst, words, n, invert,
                       offsets, nc, total);
}

extern "C" gs_status gs_gaussians_buffer_create_from_selection(gs_gaussians_buffer *src, gs_stream *s, const gs_selection *sel,
                                                               int32_t invert, gs_gaussians_buffer **out, uint64_t *count_out) {
    if (!src || !out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    *out = nullptr;
    if (count_out) *count_out = 0;
    // (the body is shared with gs_gaussians_buffer_create_converted: gs_relayout.hip)
    hipError_t e = hipSuccess;
    const gs_status rc = extract_records(src, s, sel, invert, src->sh, src->cov, out, count_out, &e);
    if (e != hipSuccess) return gs_fail(GS_ERR_HIP, (uint64_t)e, 0, 0, "extraction failed: %s", hipGetErrorString(e));
    return rc;
}

// ------------------------------------------------------------------------------------------------
// snapshots of the selected records, concatenation
// ------------------------------------------------------------------------------------------------

// The records of one selection of one buffer, with what restoring them needs: its own copy of the mask and the first
// snapshot rank of every 1024-block (the exclusive scan of the per-block counts).
struct gs_snapshot {
    gs_device *dev = nullptr;
    int sh = 0, cov = 0;
    size_t n = 0, nwords = 0, nblocks = 0;
    uint64_t count = 0;
    DevMem meta;             // nwords mask words, nblocks offsets, the scan's total (one allocation)
    size_t meta_bytes = 0;
    DevMem records;          // count records; null while count == 0
    uint32_t *words() const { return (uint32_t *)meta.ptr; }
    uint32_t *offsets() const { return words() + nwords; }
    uint32_t *total() const { return words() + nwords + nblocks; }
};

extern "C" void gs_snapshot_destroy(gs_snapshot *snap) {
    if (!snap) return;
    (void)hipSetDevice(snap->dev->ordinal);
    delete snap;      // (hipFree synchronises the device: a restore in flight finishes first)
}

extern "C" size_t gs_snapshot_len(const gs_snapshot *snap) { return snap ? snap->n : 0; }
extern "C" uint64_t gs_snapshot_count(const gs_snapshot *snap) { return snap ? snap->count : 0; }
extern "C" size_t gs_snapshot_bytes(const gs_snapshot *snap) {
    return snap ? (size_t)snap->count * (size_t)gs::pod_bytes(snap->sh, snap->cov) + snap->meta_bytes : 0;
}

// the mask, the scan and the selected records of `g` into an empty snapshot; blocks on r.st.  What it allocates is the
// snapshot's: the caller deletes that when this fails.
static gs_status snapshot_fill(const gs_gaussians_buffer *g, const RecordsAccess &r, gs_snapshot *snap) {
    GS_TRY(snap->meta.alloc(snap->meta_bytes, 0, "snapshot allocation"));
    if (!r.n) return GS_OK;
    const uint32_t nwords = (uint32_t)snap->nwords;
    // the mask is copied first and everything below reads the copy: the snapshot does not depend on the selection afterwards
    hipLaunchKernelGGL(gs::k_snapshot_mask, dim3((nwords + 255u) / 256u), dim3(256), 0, r.st, snap->words(), r.words, nwords, r.n);
    uint32_t total = 0;
    GS_TRY(extract_scan(r.st, snap->words(), r.n, 0u, snap->offsets(), snap->total(), &total));
    if (!total) return GS_OK;
    const size_t bytes = (size_t)total * pod_stride(g);
    GS_TRY(snap->records.alloc(bytes, bytes, "hipMalloc"));
    extract_copy_enqueue(r.st, g->buf->ptr, snap->records.ptr, snap->words(), r.n, 0u, snap->offsets(), (uint32_t)(pod_stride(g) / 16), total);
    hipError_t e = hipGetLastError();
    // the call is blocking anyway; a restore on any stream may follow at once
    if (e == hipSuccess) e = hipStreamSynchronize(r.st);
    if (e != hipSuccess) return gs_fail(GS_ERR_HIP, (uint64_t)e, 0, 0, "snapshot failed: %s", hipGetErrorString(e));
    snap->count = total;
    return GS_OK;
}

extern "C" gs_status gs_gaussians_buffer_snapshot(gs_gaussians_buffer *g, gs_stream *s, const gs_selection *sel, gs_snapshot **out) {
    if (out) *out = nullptr;
    if (!g || !out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    RecordsAccess r;
    GS_TRY(records_access(g, s, sel, 0, r));
    std::unique_ptr<gs_snapshot> snap(new gs_snapshot());
    snap->dev = r.dev;
    snap->sh = g->sh;
    snap->cov = g->cov;
    snap->n = r.len;
    snap->nwords = (r.len + 31) / 32;
    snap->nblocks = r.nblocks;
    snap->meta_bytes = (snap->nwords + snap->nblocks + 1) * 4;
    GS_TRY(snapshot_fill(g, r, snap.get()));
    *out = snap.release();
    return GS_OK;
}

extern "C" gs_status gs_snapshot_selection(const gs_snapshot *snap, gs_stream *s, gs_selection *sel, gs_select_op op) {
    if (!snap) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    GS_TRY(check_selection(sel, s));
    GS_TRY(check_select_op(op));
    if (snap->dev != sel->dev) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "objects belong to different devices");
    if (snap->n != sel->n) return gs_fail(GS_ERR_INVALID_ARGUMENT, snap->n, sel->n, 0, "the snapshot covers %zu Gaussians, the selection has %zu bits", snap->n, sel->n);
    return selection_combine_words(sel, s->s, op, snap->words());
}

extern "C" gs_status gs_gaussians_buffer_restore(gs_gaussians_buffer *g, gs_stream *s, gs_snapshot *snap, int32_t exchange) {
    if (!g || !snap) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    gs_device *dev = g->buf->dev;
    if (snap->dev != dev || (s && s->dev != dev)) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "objects belong to different devices");
    if (snap->sh != g->sh || snap->cov != g->cov)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "the snapshot was taken from a buffer of another layout");
    const size_t len = gs_gaussians_buffer_len(g);
    if (snap->n != len) return gs_fail(GS_ERR_INVALID_ARGUMENT, snap->n, len, 0, "the snapshot covers %zu Gaussians, the buffer has %zu", snap->n, len);
    if (!snap->count) return GS_OK;
    GS_TRY(use_device(dev));
    hipStream_t st = stream_of(dev, s);
    // a mirror rebuild in flight on another stream still reads the records; an earlier edit or restore on another stream
    // still writes them
    if (g->mirror_ready && st != g->mirror_stream) GS_HIP(hipStreamWaitEvent(st, g->mirror_ready, 0));
    GS_TRY(wait_for_edits(g, st));
    const uint32_t n = (uint32_t)len, nc = (uint32_t)(pod_stride(g) / 16), count = (uint32_t)snap->count;
    if (exchange)
        hipLaunchKernelGGL(gs::k_restore<true>, dim3((n + 255u) / 256u), dim3(256), 0, st, (uint4 *)g->buf->ptr, (uint4 *)snap->records.ptr,
                           snap->words(), n, (const uint32_t *)snap->offsets(), nc, count);
    else
        hipLaunchKernelGGL(gs::k_restore<false>, dim3((n + 255u) / 256u), dim3(256), 0, st, (uint4 *)g->buf->ptr, (uint4 *)snap->records.ptr,
                           snap->words(), n, (const uint32_t *)snap->offsets(), nc, count);
    GS_HIP(hipGetLastError());
    GS_TRY(record_edit(g, st));
    // the host does not know whether the restored records moved: the whole mirror is stale, as after a TRANSFORM edit
    g->mark_all();
    return GS_OK;
}

// (the body is shared with gs_gaussians_buffer_create_concat_as: gs_relayout.hip)
extern "C" gs_status gs_gaussians_buffer_create_concat(gs_stream *s, gs_gaussians_buffer *const *srcs, const gs_selection *const *sels,
                                                       uint32_t count, gs_gaussians_buffer **out, uint64_t *counts_out) {
    return concat_records(s, srcs, sels, count, false, 0, 0, out, counts_out);
}
