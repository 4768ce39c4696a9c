// Launch interface between the C ABI (shade_capi.cpp) and the texture stage's image-side kernels (shade_kernels.hip).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "../../include/tssplat_amd.h"

namespace tsamd {

hipError_t launch_shade(const tsamd_blend_plan &plan, const float *color, const float *background, float *out, hipStream_t stream);
hipError_t launch_shade_backward(const tsamd_blend_plan &plan, const float *grad_out, float *grad_color, hipStream_t stream);
int64_t shade_l1_workspace_bytes(int64_t pixels);
// image_out, point_sign_out / dst_sign_out may be null
hipError_t launch_shade_l1(const tsamd_blend_plan &plan, const float *color, const float *background, const float *target, int target_channels, void *workspace,
                           float *loss, float *image_out, float *point_sign_out, float *dst_sign_out, hipStream_t stream);
hipError_t launch_shade_l1_backward(const tsamd_blend_plan &plan, const float *point_sign, const float *dst_sign, const float *grad_loss, float *grad_color,
                                    hipStream_t stream);

}  // namespace tsamd
