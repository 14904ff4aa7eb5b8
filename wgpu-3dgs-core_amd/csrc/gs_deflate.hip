// gs_deflate.hip — the Huffman-only gzip member encoded on the device: gs_buffer_gzip_fast, and
// gsh::gzip_fast_device for the export (gs_export.hip).  Kernels: gs_deflate_kernels.h; the format: gs_deflate.h; the host
// encoder, which gives the same bytes: gs_deflate.cpp.
#include "gs_host.h"

#include "gs_deflate_kernels.h"

using namespace gsh;

gs_status gsh::gzip_fast_device(hipStream_t st, const uint8_t *bytes, size_t len, void *out, size_t capacity, size_t *bytes_out) {
    *bytes_out = 0;
    if (len == 0) return gs_gzip_fast(nullptr, 0, out, capacity, bytes_out);
    const uint64_t chunks64 = gs::df_chunks(len);
    if (chunks64 > 0x7fffffffull) return gs_fail(GS_ERR_INVALID_ARGUMENT, len, 0, 0, "more than 2^31 - 1 chunks of %u bytes", (unsigned)gs::DF_CHUNK);
    const uint32_t chunks = (uint32_t)chunks64;
    // [offsets: chunks + 1 x u64][sizes: chunks x u32][crcs: chunks x u32]
    // the device memory of the call, freed when it returns.  A return between the kernels and the last synchronisation (a
    // failed launch, allocation or copy) leaves kernels on it: there the frees themselves wait for the device, knowingly.
    DevMem meta, slots, body_mem;
    const size_t off_bytes = ((size_t)chunks + 1) * 8, meta_bytes = off_bytes + (size_t)chunks * 8;
    GS_TRY(meta.alloc(meta_bytes, meta_bytes, "hipMalloc"));
    uint64_t *offsets = (uint64_t *)meta.ptr;
    uint32_t *sizes = (uint32_t *)((char *)meta.ptr + off_bytes), *crcs = sizes + chunks;
    if (out) GS_TRY(slots.alloc((size_t)chunks * gs::DF_SLOT, (size_t)chunks * gs::DF_SLOT, "hipMalloc"));
    hipLaunchKernelGGL(gs::k_deflate_chunks, dim3(chunks), dim3(gs::DF_THREADS), 0, st, bytes, (uint64_t)len, (uint8_t *)slots.ptr, sizes, crcs);
    hipLaunchKernelGGL(gs::k_deflate_scan, dim3(1), dim3(gs::DF_THREADS), 0, st, (const uint32_t *)sizes, offsets, chunks);
    GS_HIP(hipGetLastError());
    uint64_t body = 0;
    hipError_t e = fetch(st, &body, offsets + chunks, 8);
    if (e != hipSuccess) return gs_fail(GS_ERR_DOWNLOAD, (uint64_t)e, 0, 0, "download failed: %s", hipGetErrorString(e));
    if (body > gs::df_bound(len) - 18u) return gs_fail(GS_ERR_HIP, body, gs::df_bound(len), 0, "the size scan returned %llu bytes for %zu", (unsigned long long)body, len);
    const size_t total = 18 + (size_t)body;
    *bytes_out = total;
    if (!out) return GS_OK;
    if (capacity < total) return gs_fail(GS_ERR_INVALID_ARGUMENT, capacity, total, 0, "output buffer too small: %zu < %zu", capacity, total);
    GS_TRY(body_mem.alloc((size_t)body, (size_t)body, "hipMalloc"));
    hipLaunchKernelGGL(gs::k_deflate_gather, dim3(chunks), dim3(gs::DF_THREADS), 0, st, (const uint8_t *)slots.ptr, (const uint32_t *)sizes,
                       (const uint64_t *)offsets, (uint8_t *)body_mem.ptr);
    GS_HIP(hipGetLastError());
    std::vector<uint32_t> host_crcs;
    try {
        host_crcs.resize(chunks);
    } catch (const std::bad_alloc &) {
        return gs_fail(GS_ERR_OUT_OF_MEMORY, (size_t)chunks * 4, 0, 0, "out of memory compressing %zu bytes", len);
    }
    uint8_t *dst = (uint8_t *)out;
    e = hipMemcpyAsync(host_crcs.data(), crcs, (size_t)chunks * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(dst + 10, body_mem.ptr, (size_t)body, hipMemcpyDeviceToHost, st);
    const hipError_t e2 = hipStreamSynchronize(st);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return gs_fail(GS_ERR_DOWNLOAD, (uint64_t)e, 0, 0, "download failed: %s", hipGetErrorString(e));
    // the chunks' CRCs fold into the member's
    gs_gzip_fast_frame(dst, (size_t)body, gs_gzip_fast_fold_crcs(host_crcs.data(), chunks, len), len);
    return GS_OK;
}

extern "C" gs_status gs_buffer_gzip_fast(gs_buffer *b, gs_stream *s, size_t offset, size_t len, void *out, size_t capacity, size_t *bytes_out) {
    if (!b || !bytes_out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    if (offset > b->bytes || len > b->bytes - offset)
        return gs_fail(GS_ERR_INVALID_ARGUMENT, offset, len, b->bytes, "range [%zu, %zu + %zu) past the %zu bytes of the buffer", offset, offset, len, b->bytes);
    if (s && s->dev != b->dev) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "objects belong to different devices");
    // the size is known only once the chunks have been encoded: a short capacity is refused after the kernels, before the copy
    GS_TRY(use_device(b->dev));
    return gzip_fast_device(stream_of(b->dev, s), (const uint8_t *)b->ptr + offset, len, out, capacity, bytes_out);
}
