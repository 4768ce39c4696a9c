// Launch interface between the C ABI (pointmesh_capi.cpp) and the exact point-to-triangle search (pointmesh_kernels.hip).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace tsamd {

constexpr int32_t kPointMeshBlock = 256;             // lanes per workgroup
constexpr int32_t kPointMeshQueriesPerLane = 1;      // a workgroup holds kPointMeshBlock * kPointMeshQueriesPerLane queries in registers (priced: DESIGN.md 15)
constexpr int32_t kPointMeshTile = 1024;             // bounding spheres per LDS tile (16 bytes each)
constexpr int32_t kPointMeshMaxChunks = 65535;       // the second grid dimension
constexpr int64_t kPointMeshTargetWorkgroups = 1024; // four per CU: the automatic rule splits the triangles until the grid has this many

inline int64_t pointmesh_query_blocks(int64_t n)
{
    const int64_t per = int64_t(kPointMeshBlock) * kPointMeshQueriesPerLane;
    return (n + per - 1) / per;
}

// the chunk count ref_chunks = 0 stands for: enough to reach kPointMeshTargetWorkgroups, never less than one tile per chunk
inline int32_t pointmesh_auto_chunks(int64_t n, int64_t n_triangles)
{
    const int64_t blocks = pointmesh_query_blocks(n);
    if (blocks <= 0 || n_triangles <= 0) return 1;
    int64_t chunks = (kPointMeshTargetWorkgroups + blocks - 1) / blocks;
    const int64_t tiles = (n_triangles + kPointMeshTile - 1) / kPointMeshTile;
    if (chunks > tiles) chunks = tiles;
    if (chunks > kPointMeshMaxChunks) chunks = kPointMeshMaxChunks;
    return int32_t(chunks < 1 ? 1 : chunks);
}

// The caller-owned workspace, 16-byte aligned, in this order (every part starts 16-byte aligned):
//   keys      [n] u64      bits(fl32 d2) << 32 | triangle, the search's result per query
//   seed_keys [n] u64      the workspace of the nearest-point search over the sphere centres
//   spheres   [T] float4   centre and radius (NaN: invalid triangle, +inf: never pruned)
//   corners   [T][3] float4
//   centres   [T][3] f32   the ref points of the seeding search (NaN: invalid triangle), padded to 16 bytes
//   seed_d2   [n] f32, seed_idx [n] i32   its outputs
struct PointMeshWorkspace {
    int64_t keys, seed_keys, spheres, corners, centres, seed_d2, seed_idx, bytes;
};
inline PointMeshWorkspace pointmesh_workspace(int64_t n, int64_t n_triangles)
{
    PointMeshWorkspace w;
    w.keys = 0;
    w.seed_keys = w.keys + 8 * n;
    w.spheres = w.seed_keys + 8 * n;
    w.corners = w.spheres + 16 * n_triangles;
    w.centres = w.corners + 48 * n_triangles;
    w.seed_d2 = w.centres + (12 * n_triangles + 15) / 16 * 16;
    w.seed_idx = w.seed_d2 + (4 * n + 15) / 16 * 16;
    w.bytes = w.seed_idx + (4 * n + 15) / 16 * 16;
    return w;
}

// n >= 1, n_triangles >= 1, 1 <= chunks <= min(n_triangles, kPointMeshMaxChunks); point_out may be null
hipError_t launch_nearest_on_mesh(const float *query, int64_t n, const float *v, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, int32_t chunks,
                                  void *workspace, float *d2_out, int32_t *tri_out, float *point_out, hipStream_t stream);

}  // namespace tsamd
