// Launch interface between the C ABI (init_capi.cpp) and the sphere-initialisation kernels (init_kernels.hip).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace tsamd {

constexpr int32_t kInitMaxGrid = 512;                 // 3 x 511^2 < 2^31: squared distances and flat indices (< 2^27) are 32-bit
constexpr int32_t kEdtSentinel = int32_t(1) << 30;    // "no false voxel in this line": loses every min, + 511^2 stays below 2^31

// bits: [batch, height, ceil(width / 32)] u32, written by the first kernel and read by the second
hipError_t launch_hull_carve(const float *alpha, int64_t batch, int32_t height, int32_t width, int32_t channels, int32_t channel, float threshold,
                             const float *mvp, int32_t grid, double lo, double step, uint32_t *bits, uint8_t *hull, hipStream_t stream);
// workspace: grid^3 i32; status: one i32, 1 when the mask has a false voxel (0: d2 is undefined)
hipError_t launch_edt_squared(const uint8_t *mask, int32_t grid, int32_t *workspace, int32_t *d2, int32_t *status, hipStream_t stream);
// keys: n_spheres + 1 u64
hipError_t launch_greedy_cover(const uint8_t *hull, const int32_t *d2, int32_t grid, int32_t n_spheres, double s2, double hs2, double m2,
                               unsigned long long *keys, uint8_t *uncovered, int32_t *flat_out, int32_t *q_out, int32_t *count_out, hipStream_t stream);

}  // namespace tsamd
