// Launch interface between the C ABI (metrics_capi.cpp) and the surface-metric kernels (metrics_kernels.hip).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace tsamd {

// ---- nearest points ----
constexpr int32_t kNearestBlock = 256;             // lanes per workgroup
constexpr int32_t kNearestQueriesPerLane = 4;      // a workgroup holds kNearestBlock * kNearestQueriesPerLane queries in registers
constexpr int32_t kNearestTile = 1024;             // ref points per LDS tile (16 bytes each)
constexpr int32_t kNearestMaxChunks = 65535;       // the second grid dimension
constexpr int64_t kNearestTargetWorkgroups = 1024; // four per CU: the automatic rule splits the ref set until the grid has this many

inline int64_t nearest_query_blocks(int64_t n) { return (n + int64_t(kNearestBlock) * kNearestQueriesPerLane - 1) / (int64_t(kNearestBlock) * kNearestQueriesPerLane); }

// the chunk count ref_chunks = 0 stands for: enough to reach kNearestTargetWorkgroups, never less than one tile per chunk
inline int32_t nearest_auto_chunks(int64_t n, int64_t m)
{
    const int64_t blocks = nearest_query_blocks(n);
    if (blocks <= 0 || m <= 0) return 1;
    int64_t chunks = (kNearestTargetWorkgroups + blocks - 1) / blocks;
    const int64_t tiles = (m + kNearestTile - 1) / kNearestTile;
    if (chunks > tiles) chunks = tiles;
    if (chunks > kNearestMaxChunks) chunks = kNearestMaxChunks;
    return int32_t(chunks < 1 ? 1 : chunks);
}

// keys: [n] u64, filled with ones by the call itself; d2_out [n] f32, idx_out [n] i32.  n >= 1, 1 <= chunks <= min(m, kNearestMaxChunks)
hipError_t launch_nearest_points(const float *query, int64_t n, const float *ref, int64_t m, int32_t chunks, uint64_t *keys, float *d2_out,
                                 int32_t *idx_out, hipStream_t stream);

// ---- surface sampler ----
constexpr int32_t kSampleWeights = 0, kSampleDraw = 1;   // phase

// weights: [T] i64, first the float64 weights, then in place the integer weights q; wmax: one u64, zero-filled by the call itself
hipError_t launch_sample_weights(const float *v, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, int64_t *weights, uint64_t *wmax,
                                 hipStream_t stream);
// prefix: [T] i64, the inclusive prefix sum of the integer weights, prefix[T - 1] > 0
hipError_t launch_sample_draw(const float *v, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, const int64_t *prefix, int64_t n_samples,
                              uint64_t seed, float *points_out, float *normals_out, int32_t *tri_out, hipStream_t stream);

}  // namespace tsamd
