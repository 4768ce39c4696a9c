// Launch interface between the C ABI (voxel_capi.cpp) and the mesh voxeliser's kernels (voxel_kernels.hip).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace tsamd {

constexpr int32_t kVoxelMinGrid = 1, kVoxelMaxGrid = 512;        // (G + 1) G^2 deposit slots per ray stay below 2^28
constexpr int32_t kVoxelSubcellBits = 10;                        // lattice units per node spacing: 2^10
constexpr int32_t kVoxelLatticeMax = 1 << 29;                    // |u| <= 2^29: every product of two differences is exact in int64
constexpr int32_t kVoxelLaneColumns = 16;                        // a face with more candidate columns is walked by its whole wave
constexpr int32_t kVoxelRuleNonzero = 0, kVoxelRulePositive = 1, kVoxelRuleOdd = 2;
// stats: twelve i64
constexpr int kVoxelStatOpen = 0;          // [3] columns whose deposits do not sum to 0, per axis
constexpr int kVoxelStatDisputed = 3;      // nodes at which the three rays disagree
constexpr int kVoxelStatInvalid = 4;       // faces with an index out of range or an unusable corner
constexpr int kVoxelStatDegenerate = 5;    // [3] valid faces of projected area 0, per axis
constexpr int kVoxelStatDeposits = 8;      // [3] covered (face, column) pairs, per axis
constexpr int kVoxelStatWaveFaces = 11;    // faces walked by a whole wave, summed over the rays
constexpr int kVoxelStats = 12;
constexpr int kVoxelStatReplicas = 64;     // copies of the record the kernels add to, so that no single word takes every wave's add
constexpr int64_t kVoxelCountBytes = int64_t(kVoxelStatReplicas) * kVoxelStats * sizeof(int64_t);

inline int64_t voxel_ray_slots(int32_t grid) { return (int64_t(grid) + 1) * grid * grid; }
// the copies of the counts, then `rays` deposit arrays
inline int64_t voxel_workspace_bytes(int32_t grid, int32_t rays) { return kVoxelCountBytes + rays * voxel_ray_slots(grid) * int64_t(sizeof(int32_t)); }

// workspace: voxel_workspace_bytes(grid, 1), 8-byte aligned.  w_out [G, G, G] i32, stats_out [12] i64 (written, not added to)
hipError_t launch_voxel_winding(const float *v, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, int32_t grid, double lo, double hi, int32_t axis,
                                void *workspace, int32_t *w_out, int64_t *stats_out, hipStream_t stream);
// workspace: voxel_workspace_bytes(grid, rays).  occ_out [G, G, G] u8 (0 / 1), stats_out [12] i64
hipError_t launch_voxel_occupancy(const float *v, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, int32_t grid, double lo, double hi, int32_t rule,
                                  int32_t rays, void *workspace, uint8_t *occ_out, int64_t *stats_out, hipStream_t stream);

}  // namespace tsamd
