// Launch interface between the C ABI (merge_capi.cpp) and the tet-sphere merge kernels (merge_kernels.hip).
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

}  // namespace tsamd
