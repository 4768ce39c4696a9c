// Launch interface between the C ABI (quality_capi.cpp) and the mesh-quality kernels (quality_kernels.hip).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace tsamd {

constexpr int32_t kQualityBlock = 256;              // Q: triangles i per workgroup, one per lane
constexpr int32_t kQualityTile = 1024;              // K: triangles j per LDS tile (two 64-bit box words each)
constexpr int32_t kQualityQueue = 128;              // surviving pairs a wave holds in LDS; 64 are evaluated whenever 64 are there
constexpr int32_t kQualityMaxChunks = 65535;        // the second grid dimension
constexpr int64_t kQualityTargetWorkgroups = 2048;  // the tiles are split over the second grid dimension until the grid has this many
constexpr int32_t kQualityLattice = 1 << 20;
constexpr int64_t kQualityMaxTriangles = (int64_t(1) << 31) / 3 - 1;   // corner ids 3 t + k stay below 2^31
constexpr int32_t kQualityStats = 8;                // int64 words of the stats record (include/tssplat_amd.h: TSAMD_QUALITY_*)

// a triangle's state
constexpr uint8_t kQualityValid = 0, kQualityDegenerate = 1, kQualityInvalid = 2;

inline int64_t quality_tiles(int64_t n_triangles) { return (n_triangles + kQualityTile - 1) / kQualityTile; }

// all pointers non-null where the count they go with is positive; n_triangles >= 1
hipError_t launch_quality_prepare(const float *v, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, double lo, double hi, uint64_t *corners,
                                  uint64_t *boxes, uint8_t *state, double *shape, int64_t *morton, hipStream_t stream);
// tile_boxes may be null (no tile is skipped); pairs may be null when max_pairs = 0
hipError_t launch_quality_pairs(const uint64_t *corners, const uint64_t *boxes, const uint8_t *state, int64_t n_triangles, uint64_t *tile_boxes,
                                int64_t max_pairs, int32_t *crossings, int64_t *pairs, int64_t *stats, hipStream_t stream);
hipError_t launch_quality_edges(const int32_t *faces, const uint8_t *state, int64_t n_triangles, int64_t n_vertices, int64_t *und_keys, int64_t *dir_keys,
                                int32_t *vertex_pairs, uint8_t *referenced, hipStream_t stream);
hipError_t launch_quality_fan_pairs(const int32_t *faces, int64_t n_triangles, const int64_t *sorted_keys, const int64_t *order, int32_t *corner_pairs,
                                    hipStream_t stream);
// Synchronises the host once per round.  rounds_out: the rounds run; returns hipSuccess with *converged = 0 when the cap was reached.
hipError_t launch_quality_union(const int32_t *pairs, int64_t n_pairs, int32_t *labels, int64_t n, int32_t *flag_dev, int64_t round_cap, int32_t *converged,
                                int64_t *rounds_out, hipStream_t stream);

}  // namespace tsamd
