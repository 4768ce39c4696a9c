// Launch interface between the C ABI (simplify_capi.cpp) and the surface simplifier's kernels (simplify_kernels.hip).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace tsamd {

constexpr int32_t kSimplifyMaxCells = 1024;                      // cell keys < 2^30
constexpr int64_t kSimplifyMaxTriangles = INT32_MAX / 3;         // three record slots per triangle, indexed with 32 bits
constexpr int64_t kSimplifySentinel = INT64_MAX;                 // an unused record slot: sorts last
constexpr int32_t kSimplifyQuadric = 0, kSimplifyMean = 1;       // placement
constexpr int32_t kSimplifyStatusRecords = 1, kSimplifyStatusOrder = 2;

// vkey_out [n_vertices] i32, records_out [3 n_triangles] i64, state_out [n_triangles] u8 (0 survives, 1 degenerate, 2 invalid)
hipError_t launch_simplify_keys(const float *v, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, int32_t cells, double lo, double hi,
                                int32_t *vkey_out, int64_t *records_out, uint8_t *state_out, hipStream_t stream);
// records: sorted; perm [3 n_triangles] i64: the slot each sorted record came from.  pos_out [3 n_triangles, 3] f32 and head_out
// [3 n_triangles] u8 (bit 0: a run starts here, bit 1: its representative was clamped) at a run's first record; run_out [3 n_triangles]
// i32 by ORIGINAL slot: the first record of the slot's run, -1 for an unused slot.  status_out: one i32
hipError_t launch_simplify_cells(const float *v, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, int32_t cells, double lo, double hi,
                                 int32_t placement, double stabilise, const int32_t *vkey, const int64_t *records, const int64_t *perm, float *pos_out,
                                 uint8_t *head_out, int32_t *run_out, int32_t *status_out, hipStream_t stream);
// tri_out [n_triangles, 3] i32: a survivor's three runs, the smallest first (-1 otherwise); the two sort keys of the triple
hipError_t launch_simplify_faces(const int32_t *run, const uint8_t *state, int64_t n_triangles, int32_t *tri_out, int64_t *key_ab_out, int64_t *key_c_out,
                                 hipStream_t stream);
// order [n_triangles] i64: the faces sorted by (triple, index).  keep_out [n_triangles] u8, used_out [3 n_triangles] u8, status_out: one i32
hipError_t launch_simplify_dedupe(const int32_t *tri, const int64_t *order, int64_t n_triangles, uint8_t *keep_out, uint8_t *used_out, int32_t *status_out,
                                  hipStream_t stream);

}  // namespace tsamd
