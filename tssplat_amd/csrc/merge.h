// Launch interface between the C ABI (merge_capi.cpp) and the tet-sphere merge kernels (merge_kernels.hip, fill_kernels.hip).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace tsamd {

constexpr int32_t kMergeMinGrid = 2;                  // a cube needs two nodes per axis
constexpr int32_t kMergeMaxGrid = 512;                // flat node indices < 2^27; 7 vertices, 12 triangles per node stay below 2^31
constexpr int64_t kMergeMaxTets = int64_t(1) << 30;   // one wave per (tet, slab), four waves per workgroup

// field: [grid^3] f32, used as the u32 key image of the maximum until the decode pass; zero-filled by the call itself
hipError_t launch_union_field(const float *tet_v, int64_t n_vertices, const int32_t *elem, int64_t n_tets, int32_t grid, double lo, double step,
                              float *field, hipStream_t stream);
// vmask / vcount / tcount: [grid^3] u8; open: one i32, zero-filled by the call itself
hipError_t launch_surface_count(const float *field, int32_t grid, float level, uint8_t *vmask, uint8_t *vcount, uint8_t *tcount, int32_t *open,
                                hipStream_t stream);
// voffset / toffset: [grid^3] i32 exclusive scans of vcount / tcount
hipError_t launch_surface_emit(const float *field, int32_t grid, double lo, double step, float level, const uint8_t *vmask, const int32_t *voffset,
                               const int32_t *toffset, int64_t n_vertices, int64_t n_triangles, float *v_out, int32_t *faces_out, hipStream_t stream);

// ---- the flood fill (fill_kernels.hip) ----
constexpr int32_t kFillCavities = 1, kFillOuter = 2;                              // mode
constexpr int32_t kFillStats = 5;                                                 // i32 words of stats, in this order:
constexpr int32_t kFillStatStatus = 0, kFillStatCavities = 1, kFillStatCavityNodes = 2, kFillStatIslands = 3, kFillStatIslandNodes = 4;
constexpr int32_t kFillStatusFindBound = 1, kFillStatusUnionBound = 2;            // status: a bounded device loop ran out of its bound

// label: [grid^3] i32, the smallest flat index of the node's component; status: one i32, zero-filled by the call itself
hipError_t launch_grid_components(const float *field, int32_t grid, float level, int32_t *label, int32_t *status, hipStream_t stream);
// workspace: [2 grid^3 + 2] i32 (8-byte aligned); out: [grid^3] f32, not the input; stats: [kFillStats] i32, zero-filled by the call itself
hipError_t launch_field_fill(const float *field, int32_t grid, float level, int32_t mode, int32_t *workspace, float *out, int32_t *stats,
                             hipStream_t stream);

}  // namespace tsamd
