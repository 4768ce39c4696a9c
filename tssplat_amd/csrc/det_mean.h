// The bitwise-repeatable mean of the renderer's fused losses (aa_kernels.hip: MSE of the alpha image; shade_kernels.hip: L1 of the
// composite): no atomics, a fixed grid, fixed trees.  The caller's accumulation kernel runs mean_blocks(n, per_block, cap) workgroups
// of kMeanBlock lanes and stores one block_sum per workgroup; mean_final_kernel adds those partials in a fixed order and stores
// float(sum / n).  The bits of a loss depend on (per_block, cap): they are part of each caller's contract.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

namespace tsamd {
namespace {

constexpr int kMeanBlock = 256;

// workgroups of the accumulation kernel (one per `per_block` elements, at most `cap`, at least one) and their partials, padded to 256 bytes
inline int mean_blocks(int64_t n, int per_block, int cap) { return int(std::min<int64_t>(cap, std::max<int64_t>(1, (n + per_block - 1) / per_block))); }
inline int64_t mean_workspace_bytes(int blocks) { return (int64_t(blocks) * 8 + 255) / 256 * 256; }

// the sum of `v` over the workgroup's kMeanBlock lanes, in every lane; `lds` holds one double per wave
__device__ __forceinline__ double block_sum(double v, double *lds)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((lds[0] + lds[1]) + (lds[2] + lds[3]));
}

__global__ __launch_bounds__(kMeanBlock) void mean_final_kernel(const double *partials, int n_partials, int64_t n, float *loss)
{
    __shared__ double lds[kMeanBlock / 64];
    double acc = 0.0;
    for (int k = threadIdx.x; k < n_partials; k += kMeanBlock) acc += partials[k];
    const double sum = block_sum(acc, lds);
    if (threadIdx.x == 0) *loss = float(sum / double(n));
}

inline hipError_t launch_mean_final(const void *workspace, int blocks, int64_t n, float *loss, hipStream_t stream)
{
    hipLaunchKernelGGL(mean_final_kernel, dim3(1), dim3(kMeanBlock), 0, stream, static_cast<const double *>(workspace), blocks, n, loss);
    return hipGetLastError();
}

}  // namespace
}  // namespace tsamd
