// gs_export.hip — a buffer, or a selection of it, as PLY vertices, an SPZ payload or a complete file image, encoded on the
// device.  Kernels: gs_export_kernels.h; the extraction scan is gs_edit.hip's, the gzip member gs_spz.cpp's.
#include "gs_host.h"

#include "gs_export_kernels.h"

using namespace gsh;

typedef void (*export_ply_fn)(const uint4 *, uint2 *, const uint32_t *, uint32_t, uint32_t, const uint32_t *, uint32_t, uint64_t, uint64_t);
typedef void (*export_spz_fn)(const uint4 *, gs::SpzOut, const uint32_t *, uint32_t, uint32_t, const uint32_t *, uint64_t);
static export_ply_fn k_tbl_export_ply[3] = {gs::k_export_ply<0>, gs::k_export_ply<1>, gs::k_export_ply<2>};
static export_spz_fn k_tbl_export_spz[3] = {gs::k_export_spz<0>, gs::k_export_spz<1>, gs::k_export_spz<2>};

// what every export starts with: the layouts that can be exported, then the prelude and the scan of an extraction
static gs_status export_begin(gs_gaussians_buffer *g, gs_stream *s, const gs_selection *sel, int32_t invert, ExtractScan &x) {
    if (!g) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null buffer");
    // the layouts gs_gaussians_buffer_download_gaussians accepts, and its error for the others
    if (g->sh == GS_SH_NONE || g->cov != GS_COV3D_ROT_SCALE)
        return gs_unpack_to_gaussian((gs_sh_config)g->sh, (gs_cov3d_config)g->cov, nullptr, 0, nullptr);
    return extract_begin(g, s, sel, invert, x);
}

// GS3D_EXPORT_SLICE (records, a multiple of 1024; tests cross slice boundaries with it): the source records one kernel of the
// PLY export covers.  Default: the 2 Mi records of gs_gaussians_buffer_download_gaussians.
static size_t export_slice() {
    const long v = switches().export_slice;
    return v >= 1024 ? (size_t)v / 1024 * 1024 : (size_t)2 << 20;
}

// The x.total vertices of the scan -> out (host memory of any alignment), in caller order.  The source is walked in slices of
// whole 1024-blocks; the vertices of slice k are ranks [offsets[b0], offsets[b1]) — the offsets come to the host once — and
// land in one of TWO staging buffers.  The kernel of slice k + 1 is enqueued on the caller's stream BEFORE the device-to-host
// copy of slice k is issued on a stream of its own (a copy into pageable memory may hold the host until it is done), so the
// kernel can run under that copy; events order a staging buffer's kernel, its copy and the next kernel that overwrites it.
// That the two overlap on the device was not measured; at 0.2 ms of kernel per 30 ms of copy the total does not depend on it.
static gs_status export_ply_records(gs_gaussians_buffer *g, ExtractScan &x, uint8_t *out) {
    if (!x.total) return GS_OK;
    const size_t slice = export_slice();
    const uint32_t slices = (uint32_t)(((size_t)x.n + slice - 1) / slice);
    const int nbuf = slices > 1 ? 2 : 1;
    std::vector<uint32_t> offsets((size_t)x.nblocks + 1);
    hipError_t e = fetch(x.st, offsets.data(), x.scan.ptr, offsets.size() * 4);
    if (e != hipSuccess) return gs_fail(GS_ERR_DOWNLOAD, (uint64_t)e, 0, 0, "export failed: %s", hipGetErrorString(e));
    const size_t blocks_per_slice = slice / gs::PLANAR_BLOCK;
    // a staging buffer holds the most vertices any slice selects
    size_t most = 0;
    for (uint32_t k = 0; k < slices; k++) {
        const size_t b0 = (size_t)k * blocks_per_slice, b1 = b0 + blocks_per_slice < x.nblocks ? b0 + blocks_per_slice : x.nblocks;
        if (offsets[b1] < offsets[b0] || offsets[b1] - offsets[b0] > (b1 - b0) * gs::PLANAR_BLOCK)
            return gs_fail(GS_ERR_HIP, b0, b1, 0, "selection scan returned offsets out of order");
        if (offsets[b1] - offsets[b0] > most) most = offsets[b1] - offsets[b0];
    }
    if (offsets[x.nblocks] != x.total) return gs_fail(GS_ERR_HIP, offsets[x.nblocks], x.total, 0, "selection scan returned offsets out of order");
    // Declared in the order the return has to undo: the copy stream goes first, then the events, then the memory.  Nothing is
    // enqueued while they are made (the fetch above has just drained x.st), so a failure here returns at once.
    const size_t rec = sizeof(gs_ply_gaussian_pod);
    DevMem staging[2];
    Event encoded[2], copied[2];
    Stream copy;
    for (int i = 0; i < nbuf; i++) {
        if ((e = staging[i].alloc_raw(most * rec)) != hipSuccess)
            return gs_fail(GS_ERR_OUT_OF_MEMORY, most * rec, 0, 0, "hipMalloc failed: %s", hipGetErrorString(e));
        if ((e = encoded[i].create()) != hipSuccess || (e = copied[i].create()) != hipSuccess)
            return gs_fail(GS_ERR_HIP, (uint64_t)e, 0, 0, "hipEventCreate failed: %s", hipGetErrorString(e));
    }
    if (nbuf > 1 && (e = copy.create()) != hipSuccess)
        return gs_fail(GS_ERR_HIP, (uint64_t)e, 0, 0, "hipStreamCreate failed: %s", hipGetErrorString(e));
    const hipStream_t copy_st = copy.s, cst = copy_st ? copy_st : x.st;
    gs_status rc = GS_OK;
    bool used[2] = {false, false};
    int b = 0;
    // the copy of the slice encoded last, issued once the next slice's kernel has been enqueued
    int pending = -1;
    uint64_t pending_rank0 = 0, pending_count = 0;
    auto issue_copy = [&]() -> hipError_t {
        if (pending < 0) return hipSuccess;
        hipError_t ce = copy_st ? hipStreamWaitEvent(copy_st, encoded[pending].e, 0) : hipSuccess;
        if (ce == hipSuccess)
            ce = hipMemcpyAsync(out + pending_rank0 * rec, staging[pending].ptr, (size_t)pending_count * rec, hipMemcpyDeviceToHost, cst);
        if (ce == hipSuccess && copy_st) ce = hipEventRecord(copied[pending].e, copy_st);
        pending = -1;
        return ce;
    };
    for (uint32_t k = 0; k < slices && rc == GS_OK; k++) {
        const size_t b0 = (size_t)k * blocks_per_slice, b1 = b0 + blocks_per_slice < x.nblocks ? b0 + blocks_per_slice : x.nblocks;
        const uint64_t rank0 = offsets[b0], rank_end = offsets[b1];
        if (rank_end == rank0) continue;
        const uint32_t first = (uint32_t)(b0 * gs::PLANAR_BLOCK);
        const uint32_t end = b1 * gs::PLANAR_BLOCK < x.n ? (uint32_t)(b1 * gs::PLANAR_BLOCK) : x.n;
        // the kernel overwrites staging[b]: its previous copy (issued two slices ago) must have left
        e = used[b] && copy_st ? hipStreamWaitEvent(x.st, copied[b].e, 0) : hipSuccess;
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_tbl_export_ply[g->sh], dim3((end - first + gs::EXPORT_GROUP - 1u) / gs::EXPORT_GROUP), dim3(gs::EXPORT_GROUP),
                               0, x.st, (const uint4 *)g->buf->ptr, (uint2 *)staging[b].ptr, x.words, x.n, x.inv, x.offsets(),
                               first, rank0, rank_end);
            e = hipGetLastError();
        }
        if (e == hipSuccess && copy_st) e = hipEventRecord(encoded[b].e, x.st);
        if (e == hipSuccess) e = issue_copy();      // the previous slice's, into the other staging buffer
        if (e != hipSuccess) {
            rc = gs_fail(GS_ERR_DOWNLOAD, (uint64_t)e, 0, 0, "export failed: %s", hipGetErrorString(e));
            break;
        }
        pending = b;
        pending_rank0 = rank0;
        pending_count = rank_end - rank0;
        used[b] = true;
        b ^= nbuf - 1;
    }
    if (rc == GS_OK && (e = issue_copy()) != hipSuccess) rc = gs_fail(GS_ERR_DOWNLOAD, (uint64_t)e, 0, 0, "export failed: %s", hipGetErrorString(e));
    // the staging buffers are freed at the return and the caller reads `out`: wait for everything, on every path from the loop
    e = hipStreamSynchronize(x.st);
    if (copy_st) {
        const hipError_t e2 = hipStreamSynchronize(copy_st);
        if (e == hipSuccess) e = e2;
    }
    if (e != hipSuccess && rc == GS_OK) rc = gs_fail(GS_ERR_DOWNLOAD, (uint64_t)e, 0, 0, "export failed: %s", hipGetErrorString(e));
    return rc;
}

extern "C" gs_status gs_gaussians_buffer_export_ply(gs_gaussians_buffer *g, gs_stream *s, const gs_selection *sel, int32_t invert,
                                                    gs_ply_gaussian_pod *out, size_t capacity, uint64_t *count_out) {
    if (!g || !count_out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    *count_out = 0;
    ExtractScan x;
    GS_TRY(export_begin(g, s, sel, invert, x));
    *count_out = x.total;
    if (!out) return GS_OK;
    if (capacity < x.total)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, capacity, x.total, 0, "output buffer too small: %zu < %u records", capacity, x.total);
    return export_ply_records(g, x, (uint8_t *)out);
}

// The x.total records of the scan as a decompressed SPZ payload in `payload` (host, `bytes` long: gs_spz_encode_layout's size
// for x.total records).  The whole payload is built on the device (at most 16 + 65 bytes per record) and comes over in one copy.
// the six columns of the x.total > 0 records into dev_payload (device, `bytes` long; its first 16 bytes are the header's and
// are left alone).  Only enqueues.
static hipError_t export_spz_columns(gs_gaussians_buffer *g, ExtractScan &x, const gs_spz_header &h, const size_t off[6], uint32_t ncoef,
                                     uint32_t bucket, uint8_t *dev_payload) {
    gs::SpzOut o;
    for (int c = 0; c < 6; c++) {
        o.col[c] = dev_payload + off[c];
        o.width[c] = gs::spz_col_bytes(c, h.version, ncoef);
    }
    o.version = h.version;
    o.fractional_bits = h.fractional_bits;
    o.ncoef = ncoef;
    o.bucket = bucket;
    hipLaunchKernelGGL(k_tbl_export_spz[g->sh], dim3((x.n + gs::EXPORT_GROUP - 1u) / gs::EXPORT_GROUP), dim3(gs::EXPORT_GROUP), 0, x.st,
                       (const uint4 *)g->buf->ptr, o, x.words, x.n, x.inv, x.offsets(), (uint64_t)x.total);
    return hipGetLastError();
}

static gs_status export_spz_payload(gs_gaussians_buffer *g, ExtractScan &x, const gs_spz_header &h, const size_t off[6], uint32_t ncoef,
                                    uint32_t bucket, uint8_t *payload, size_t bytes) {
    std::memcpy(payload, &h, 16);
    if (!x.total) return GS_OK;
    DevMem mem;
    GS_TRY(mem.alloc(bytes, bytes, "hipMalloc"));
    uint8_t *dev_payload = (uint8_t *)mem.ptr;
    hipError_t e = export_spz_columns(g, x, h, off, ncoef, bucket, dev_payload);
    if (e == hipSuccess) e = hipMemcpyAsync(payload + 16, dev_payload + 16, bytes - 16, hipMemcpyDeviceToHost, x.st);
    const hipError_t e2 = hipStreamSynchronize(x.st);      // whatever was enqueued: the payload is freed at the return
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return gs_fail(GS_ERR_DOWNLOAD, (uint64_t)e, 0, 0, "export failed: %s", hipGetErrorString(e));
    return GS_OK;
}

// both SPZ exports: the payload into `raw` when it has to be compressed, else straight into `out`
static gs_status export_spz(gs_gaussians_buffer *g, gs_stream *s, const gs_selection *sel, int32_t invert, const gs_spz_options *options,
                            bool compress, void *out, size_t capacity, size_t *bytes_out) {
    if (!g || !bytes_out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    *bytes_out = 0;
    gs_spz_options dflt;
    gs_spz_options_default(&dflt);
    const gs_spz_options *opt = options ? options : &dflt;
    ExtractScan x;
    GS_TRY(export_begin(g, s, sel, invert, x));
    gs_spz_header h;
    size_t off[6], bytes = 0;
    uint32_t ncoef = 0, bucket = 0;
    GS_TRY(gs_spz_encode_layout(x.total, opt, &h, off, &ncoef, &bucket, &bytes));
    if (!compress) {
        *bytes_out = bytes;
        if (!out) return GS_OK;
        if (capacity < bytes) return gs_fail(GS_ERR_INVALID_ARGUMENT, capacity, bytes, 0, "output buffer too small: %zu < %zu", capacity, bytes);
        return export_spz_payload(g, x, h, off, ncoef, bucket, (uint8_t *)out, bytes);
    }
    // the size of the gzip member is known only once it exists: a size query compresses too
    std::vector<uint8_t> raw;
    try {
        raw.resize(bytes);
    } catch (const std::bad_alloc &) {
        return gs_fail(GS_ERR_OUT_OF_MEMORY, bytes, 0, 0, "out of memory encoding SPZ data");
    }
    GS_TRY(export_spz_payload(g, x, h, off, ncoef, bucket, raw.data(), bytes));
    return gs_spz_compress(raw.data(), raw.size(), out, out ? capacity : 0, bytes_out);
}

extern "C" gs_status gs_gaussians_buffer_export_spz_decompressed(gs_gaussians_buffer *g, gs_stream *s, const gs_selection *sel, int32_t invert,
                                                                 const gs_spz_options *options, void *out, size_t capacity, size_t *bytes_out) {
    return export_spz(g, s, sel, invert, options, false, out, capacity, bytes_out);
}

extern "C" gs_status gs_gaussians_buffer_export_spz(gs_gaussians_buffer *g, gs_stream *s, const gs_selection *sel, int32_t invert,
                                                    const gs_spz_options *options, void *out, size_t capacity, size_t *bytes_out) {
    return export_spz(g, s, sel, invert, options, true, out, capacity, bytes_out);
}

// The member of gs_gzip_fast around the payload of export_spz: the payload never leaves the device.
extern "C" gs_status gs_gaussians_buffer_export_spz_fast(gs_gaussians_buffer *g, gs_stream *s, const gs_selection *sel, int32_t invert,
                                                         const gs_spz_options *options, void *out, size_t capacity, size_t *bytes_out) {
    if (!g || !bytes_out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    *bytes_out = 0;
    gs_spz_options dflt;
    gs_spz_options_default(&dflt);
    const gs_spz_options *opt = options ? options : &dflt;
    ExtractScan x;
    GS_TRY(export_begin(g, s, sel, invert, x));
    gs_spz_header h;
    size_t off[6], bytes = 0;
    uint32_t ncoef = 0, bucket = 0;
    GS_TRY(gs_spz_encode_layout(x.total, opt, &h, off, &ncoef, &bucket, &bytes));
    if (!x.total) return gs_gzip_fast(&h, 16, out, out ? capacity : 0, bytes_out);      // the header alone: the same bytes from the host
    DevMem mem;
    GS_TRY(mem.alloc(bytes, bytes, "hipMalloc"));
    uint8_t *dev_payload = (uint8_t *)mem.ptr;
    hipError_t e = hipMemcpyAsync(dev_payload, &h, 16, hipMemcpyHostToDevice, x.st);
    if (e == hipSuccess) e = export_spz_columns(g, x, h, off, ncoef, bucket, dev_payload);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(x.st);      // the header's copy may be in flight, and the payload is freed at the return
        return gs_fail(GS_ERR_HIP, (uint64_t)e, 0, 0, "export failed: %s", hipGetErrorString(e));
    }
    // (a member that fails after its kernels returns without a wait: the frees of its scratch and of the payload wait)
    return gzip_fast_device(x.st, dev_payload, bytes, out, out ? capacity : 0, bytes_out);
}

extern "C" gs_status gs_gaussians_buffer_write(gs_gaussians_buffer *g, gs_stream *s, const gs_selection *sel, int32_t invert,
                                               gs_gaussians_source source, void *out, size_t capacity, size_t *bytes_out) {
    if (!g || !bytes_out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    *bytes_out = 0;
    switch (source) {
    case GS_SOURCE_PLY: {
        ExtractScan x;
        GS_TRY(export_begin(g, s, sel, invert, x));
        const std::string hdr = gs_ply_header(x.total);
        const size_t bytes = hdr.size() + (size_t)x.total * sizeof(gs_ply_gaussian_pod);
        *bytes_out = bytes;
        if (!out) return GS_OK;
        if (capacity < bytes) return gs_fail(GS_ERR_INVALID_ARGUMENT, capacity, bytes, 0, "output buffer too small: %zu < %zu", capacity, bytes);
        std::memcpy(out, hdr.data(), hdr.size());
        return export_ply_records(g, x, (uint8_t *)out + hdr.size());      // the vertices land directly behind the header
    }
    case GS_SOURCE_SPZ: return export_spz(g, s, sel, invert, nullptr, true, out, capacity, bytes_out);
    default: return gs_fail(GS_ERR_INVALID_ARGUMENT, (uint64_t)source, 0, 0, "cannot write Internal Gaussians to buffer");
    }
}
