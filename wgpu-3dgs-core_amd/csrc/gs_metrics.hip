// gs_metrics.hip — image metrics: gs_image_compare.  Kernels: gs_metrics_kernels.h.
#include "gs_host.h"

#include "gs_metrics_kernels.h"

using namespace gsh;

static_assert(sizeof(gs::MetricsOut) == sizeof(gs_image_metrics), "the device result is a gs_image_metrics");
static_assert(offsetof(gs::MetricsOut, max_abs_at) == offsetof(gs_image_metrics, max_abs_at) &&
                  offsetof(gs::MetricsOut, ssim_finite) == offsetof(gs_image_metrics, ssim_finite),
              "the device result is a gs_image_metrics");

extern "C" gs_status gs_image_compare(gs_device *dev, gs_stream *s, const float *a, const float *b, uint32_t width, uint32_t height,
                                      const gs_image_compare_desc *desc, gs_image_metrics *out) {
    // every check comes before the device is touched
    if (!dev || !a || !b || !out) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "null argument");
    if (!width || !height) return gs_fail(GS_ERR_INVALID_ARGUMENT, width, height, 0, "an image of %u x %u pixels", (unsigned)width, (unsigned)height);
    const uint64_t npix = (uint64_t)width * height;
    if (npix > 0xfffffffeull) return gs_fail(GS_ERR_INVALID_ARGUMENT, width, height, 0, "more than 2^32 - 2 pixels");
    if (((uintptr_t)a | (uintptr_t)b) & 15u) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "an image is not 16-byte aligned");
    uint32_t flags = 0u;
    float L = 1.0f, *err_plane = nullptr, *ssim_plane = nullptr;
    if (desc) {
        flags = desc->flags;
        L = desc->data_range;
        err_plane = desc->err_plane;
        ssim_plane = desc->ssim_plane;
        if (flags & ~(uint32_t)GS_COMPARE_SSIM) return gs_fail(GS_ERR_INVALID_ARGUMENT, flags, 0, 0, "unknown flags 0x%x", (unsigned)flags);
        for (uint32_t r : desc->reserved)
            if (r) return gs_fail(GS_ERR_INVALID_ARGUMENT, r, 0, 0, "gs_image_compare_desc.reserved must be 0");
        if (!std::isfinite(L) || !(L > 0.0f)) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "data_range must be finite and positive");
        if (((uintptr_t)err_plane | (uintptr_t)ssim_plane) & 3u) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "a plane is not 4-byte aligned");
        if (ssim_plane && !(flags & GS_COMPARE_SSIM)) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "ssim_plane needs GS_COMPARE_SSIM");
    }
    if (s && s->dev != dev) return gs_fail(GS_ERR_INVALID_ARGUMENT, 0, 0, 0, "objects belong to different devices");
    const bool ssim = (flags & GS_COMPARE_SSIM) != 0u;
    // C1 = (0.01 L)^2, C2 = (0.03 L)^2: two rounded multiplies each
    const float k1 = 0.01f * L, k2 = 0.03f * L;
    const float C1 = k1 * k1, C2 = k2 * k2;

    GS_TRY(use_device(dev));
    hipStream_t st = stream_of(dev, s);
    // 32 x 16 tiles; W H < 2^32, so there are fewer than 2^29 of them.  A workgroup takes every nblocks-th one.
    const uint32_t tiles_x = (uint32_t)(((uint64_t)width + gs::MET_TW - 1u) / gs::MET_TW);
    const uint32_t tiles_y = (uint32_t)(((uint64_t)height + gs::MET_TH - 1u) / gs::MET_TH);
    const uint64_t ntiles = (uint64_t)tiles_x * tiles_y;
    const uint32_t nblocks = (uint32_t)(ntiles < gs::MET_MAX_GROUPS ? ntiles : gs::MET_MAX_GROUPS);
    // [the result, 256 bytes][11 x nblocks doubles][4 x nblocks keys][6 x nblocks words]
    const size_t d_bytes = (size_t)gs::MET_D_FIELDS * nblocks * 8, k_bytes = (size_t)gs::MET_K_FIELDS * nblocks * 8,
                 u_bytes = (size_t)gs::MET_U_FIELDS * nblocks * 4;
    // the device keeps the scratch of the call: calls on one device take turns
    std::lock_guard<std::mutex> lock(dev->metrics_mu);
    GS_TRY(dev_reserve(dev->metrics_scratch, 256 + d_bytes + k_bytes + u_bytes));
    char *base = (char *)dev->metrics_scratch.ptr;
    gs::MetricsOut *dout = (gs::MetricsOut *)base;
    double *part_d = (double *)(base + 256);
    unsigned long long *part_k = (unsigned long long *)(base + 256 + d_bytes);
    uint32_t *part_u = (uint32_t *)(base + 256 + d_bytes + k_bytes);
    hipLaunchKernelGGL(ssim ? gs::k_metrics_tiles<true> : gs::k_metrics_tiles<false>, dim3(nblocks), dim3(256), 0, st, (const float4 *)a,
                       (const float4 *)b, width, height, tiles_x, (uint32_t)ntiles, C1, C2, err_plane, ssim_plane, part_d, part_k, part_u,
                       nblocks);
    hipLaunchKernelGGL(gs::k_metrics_finish, dim3(1), dim3(256), 0, st, (const double *)part_d, (const unsigned long long *)part_k,
                       (const uint32_t *)part_u, nblocks, npix, dout);
    GS_HIP(hipGetLastError());
    gs_image_metrics res;
    GS_HIP(hipMemcpyAsync(&res, dout, sizeof(res), hipMemcpyDeviceToHost, st));
    hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return gs_fail(GS_ERR_DOWNLOAD, (uint64_t)e, 0, 0, "download failed: %s", hipGetErrorString(e));
    *out = res;
    return GS_OK;
}
