// gs_neighbor_grid.h — what the kernel headers that walk the sorted cell grid share (gs_neighbor_kernels.h: DESIGN.md
// §3.11; gs_component_kernels.h: §3.16; gs_knn_kernels.h: §3.18): the layout of a cell key and the wave broadcast.  No kernel lives here.
#pragma once

#include "gs_device_common.h"

namespace gs {

constexpr uint32_t NB_CELL_BITS = 21u, NB_CELL_MAX = (1u << NB_CELL_BITS) - 1u;
constexpr uint64_t NB_KEY_NONE = ~0ull;           // not a point: sorts behind every cell and is never visited
constexpr uint32_t NB_NOT_A_POINT = 0xffffffffu;  // k_nb_count<true>: the count word of such a Gaussian (a count is < 2^32 - 16)
constexpr uint32_t NB_SPAN = 6u;                  // the queries that search together lie in one row, at most this many cells apart

__device__ __forceinline__ uint32_t nb_readlane(uint32_t v, uint32_t l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l); }
__device__ __forceinline__ float nb_readlane_f(float v, uint32_t l) { return u2f(nb_readlane(f2u(v), l)); }

// The cell side from the bounding box (k_bbox_final) and the radius, in binary64:
//   h = max(r (1 + 2^-10), extent 2^-21 (1 + 2^-10), 2^-62)
// r (1 + 2^-10): the margin of DESIGN.md §3.11; extent 2^-21: 21 bits per axis cover the box WITHOUT a cap on the
// resolution where r is larger (a far outlier only grows the box); 2^-62: r = 0, and every difference whose square is
// subnormal in binary32 (< 2^-63) stays inside one cell side.  No point: lo = 0.
__device__ __forceinline__ double nb_grid_side(const float *__restrict__ bbox, float radius, double lo[3]) {
    double ext = 0.0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const bool any = bbox[a] <= bbox[3 + a];
        lo[a] = any ? (double)bbox[a] : 0.0;
        ext = fmax(ext, any ? (double)bbox[3 + a] - (double)bbox[a] : 0.0);
    }
    const double margin = 1.0 + 0x1p-10;
    return fmax(fmax((double)radius * margin, ext * 0x1p-21 * margin), 0x1p-62);
}
// ... and 1 / h, which the keys are made with
__device__ __forceinline__ double nb_grid(const float *__restrict__ bbox, float radius, double lo[3]) {
    return 1.0 / nb_grid_side(bbox, radius, lo);
}

__device__ __forceinline__ uint32_t nb_cell(float v, double lo, double inv_h) {
    const double u = ((double)v - lo) * inv_h;      // >= 0: lo is the smallest coordinate of a point
    return u >= (double)NB_CELL_MAX ? NB_CELL_MAX : (u > 0.0 ? (uint32_t)u : 0u);
}

}  // namespace gs
