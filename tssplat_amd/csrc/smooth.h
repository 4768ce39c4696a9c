// Launch interface between the C ABI (smooth_capi.cpp) and the surface-smoothing kernels (smooth_kernels.hip).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace tsamd {

constexpr int32_t kSmoothBlock = 256;                                   // lanes per workgroup: one face, key position or vertex each
constexpr int64_t kSmoothMaxTriangles = (int64_t(1) << 31) / 6 - 1;     // six directed keys per face, positions below 2^31
constexpr int64_t kSmoothSentinel = INT64_MAX;                          // the key of an invalid face: sorts last
constexpr int32_t kSmoothMaxIterations = 4096;

// include/tssplat_amd.h: TSAMD_SMOOTH_*
constexpr int32_t kSmoothTaubin = 0, kSmoothTangential = 1;
constexpr uint8_t kSmoothMoves = 0, kSmoothHeldOther = 1, kSmoothHeldPinned = 2, kSmoothHeldIrregular = 3;

// The connectivity a half-step walks.  offsets / face_offsets: [n_vertices + 1]; the kernels never trust an entry: a row outside
// 0 .. n_neighbours (n_face_entries), a neighbour outside 0 .. n_vertices - 1 or a face outside 0 .. n_triangles - 1 holds the vertex.
struct SmoothMesh {
    const int32_t *offsets;
    const int32_t *neighbours;
    int64_t n_neighbours;
    const int32_t *face_offsets;                                        // tangential only
    const int32_t *faces_of;
    int64_t n_face_entries;
    const int32_t *faces;
    int64_t n_triangles;
    int64_t n_vertices;
};

// all pointers non-null where the count they go with is positive
hipError_t launch_smooth_keys(const int32_t *faces, int64_t n_triangles, int64_t n_vertices, uint8_t *valid, int64_t *edge_keys, int64_t *face_keys,
                              hipStream_t stream);
hipError_t launch_smooth_rows(const int64_t *sorted_keys, int64_t n_keys, int64_t n_vertices, uint8_t *head, uint8_t *irregular, hipStream_t stream);
hipError_t launch_smooth_classify(const float *v, const SmoothMesh &mesh, const uint8_t *irregular, const uint8_t *pinned, int32_t boundary_free,
                                  uint8_t *cls, hipStream_t stream);
// One half-step src -> dst (different buffers of n_vertices x stride float64, stride 3 or 4).  v0: the float32 input the clamp is
// centred on, null for no clamp.
hipError_t launch_smooth_step(const double *src, double *dst, int32_t stride, const SmoothMesh &mesh, const uint8_t *cls, int32_t mode, double coef,
                              const float *v0, double max_move, hipStream_t stream);

}  // namespace tsamd
