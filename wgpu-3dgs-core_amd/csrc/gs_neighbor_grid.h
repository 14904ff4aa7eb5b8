// gs_neighbor_grid.h — what the two kernel headers that walk the sorted cell grid share (gs_neighbor_kernels.h: DESIGN.md
// §3.11; gs_component_kernels.h: §3.16): the layout of a cell key and the wave broadcast.  No kernel lives here.
#pragma once

#include "gs_device_common.h"

namespace gs {

constexpr uint32_t NB_CELL_BITS = 21u, NB_CELL_MAX = (1u << NB_CELL_BITS) - 1u;
constexpr uint64_t NB_KEY_NONE = ~0ull;           // not a point: sorts behind every cell and is never visited
constexpr uint32_t NB_NOT_A_POINT = 0xffffffffu;  // k_nb_count<true>: the count word of such a Gaussian (a count is < 2^32 - 16)
constexpr uint32_t NB_SPAN = 6u;                  // the queries that search together lie in one row, at most this many cells apart

__device__ __forceinline__ uint32_t nb_readlane(uint32_t v, uint32_t l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l); }
__device__ __forceinline__ float nb_readlane_f(float v, uint32_t l) { return u2f(nb_readlane(f2u(v), l)); }

}  // namespace gs
