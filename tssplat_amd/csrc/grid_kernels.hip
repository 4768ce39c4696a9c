// gfx950 kernels of the multiresolution hash-grid encoding (grid.h; semantics: tests/hashgrid_oracle.py).
//
//   grid_encode_kernel               forward, one lane per (point, level), the level the slow grid dimension (as tiny-cuda-nn's
//                                    kernel_grid): the waves in flight read one level's table, which stays in L2 / the MALL
//   grid_backward_params_lds_kernel  dL/dparams of the coarse levels whose table fits in LDS (level 0: 32 KB, level 1: 110 KB at
//                                    F = 2): a few workgroups per CU accumulate with LDS float atomics over a grid-stride
//                                    loop, then add the table into global memory with contiguous 256-B atomic wave-instructions
//   grid_backward_params_kernel      dL/dparams of the other levels: one global_atomic_add_f32 per feature, after the lanes of
//                                    a wave that hit the same entry with the same corner (neighbouring pixels in one cell)
//                                    summed their adds on chip
//   grid_backward_x_kernel           dL/dx, one lane per point looping over the levels: plain stores, bitwise repeatable
//
// The forward and dL/dx are bitwise deterministic (fixed summation order); dL/dparams is a float-atomic sum and may differ in
// the last bits from run to run (tiny-cuda-nn's is too).
#include <hip/hip_runtime.h>

#include "grid.h"

namespace tsamd {
namespace {

constexpr int kBlock = 256;
constexpr int kLdsBlock = 1024;
constexpr uint32_t kInvalid = 0xffffffffu;

template <int F>
__device__ __forceinline__ void load_feat(const float *p, float (&v)[F])
{
    if constexpr (F == 1) {
        v[0] = p[0];
    } else if constexpr (F == 2) {
        const float2 t = *reinterpret_cast<const float2 *>(p);
        v[0] = t.x;
        v[1] = t.y;
    } else {
#pragma unroll
        for (int k = 0; k < F; k += 4) {
            const float4 t = *reinterpret_cast<const float4 *>(p + k);
            v[k] = t.x;
            v[k + 1] = t.y;
            v[k + 2] = t.z;
            v[k + 3] = t.w;
        }
    }
}

template <int F>
__device__ __forceinline__ void store_feat(float *p, const float (&v)[F])
{
    if constexpr (F == 1) {
        p[0] = v[0];
    } else if constexpr (F == 2) {
        *reinterpret_cast<float2 *>(p) = make_float2(v[0], v[1]);
    } else {
#pragma unroll
        for (int k = 0; k < F; k += 4) *reinterpret_cast<float4 *>(p + k) = make_float4(v[k], v[k + 1], v[k + 2], v[k + 3]);
    }
}

// pos = fmaf(scale, x, 0.5f); cell = (uint32)(int)floorf(pos); frac = pos - floorf(pos) (no clamping: a negative cell wraps)
struct Cell {
    uint32_t c[3];
    float f[3];
};

__device__ __forceinline__ Cell cell_of(const float (&x)[3], float scale)
{
    Cell cl;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float pos = fmaf(scale, x[d], 0.5f);
        const float fl = floorf(pos);
        cl.c[d] = uint32_t(int(fl));
        cl.f[d] = pos - fl;
    }
    return cl;
}

// tiny-cuda-nn grid_index: dense stride index or the coherent prime hash, uint32 wrap-around, then % entries
__device__ __forceinline__ uint32_t corner_index(const Cell &cl, int corner, uint32_t res, uint32_t entries, bool hashed)
{
    const uint32_t x = cl.c[0] + (corner & 1), y = cl.c[1] + ((corner >> 1) & 1), z = cl.c[2] + ((corner >> 2) & 1);
    const uint32_t i = hashed ? (x ^ (y * 2654435761u) ^ (z * 805459861u)) : (x + y * res + z * (res * res));
    return (entries & (entries - 1)) == 0 ? (i & (entries - 1)) : (i % entries);
}

__device__ __forceinline__ float corner_weight(const Cell &cl, int corner)
{
    const float wx = (corner & 1) ? cl.f[0] : 1.0f - cl.f[0];
    const float wy = (corner & 2) ? cl.f[1] : 1.0f - cl.f[1];
    const float wz = (corner & 4) ? cl.f[2] : 1.0f - cl.f[2];
    return wx * wy * wz;
}

__device__ __forceinline__ void load_point(const float *x, int64_t i, float (&p)[3])
{
    p[0] = x[3 * i];
    p[1] = x[3 * i + 1];
    p[2] = x[3 * i + 2];
}

// Sums v over the run of consecutive lanes holding the same key; returns true on the run's first lane, which then holds the
// run's sum.  Every lane of the wave must call it (inactive lanes pass kInvalid and zeros).  Hillis-Steele suffix scan
// restricted to the run; skipped (one ballot) when no two neighbouring lanes share a key.
template <int F>
__device__ __forceinline__ bool combine_runs(uint32_t key, float (&v)[F])
{
    const int lane = __lane_id();
    const uint32_t prev = __shfl_up(key, 1);
    const bool head = lane == 0 || prev != key;
    const unsigned long long heads = __ballot(head);
    if (heads == ~0ull) return true;
    const unsigned long long rest = lane == 63 ? 0ull : (heads >> (lane + 1));
    const int end = rest ? lane + __ffsll(static_cast<long long>(rest)) - 1 : 63;   // last lane of this lane's run
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
        for (int f = 0; f < F; ++f) {
            const float o = __shfl_down(v[f], d);
            if (lane + d <= end) v[f] += o;
        }
    }
    return head;
}

template <int F>
__global__ __launch_bounds__(kBlock) void grid_encode_kernel(const float *__restrict__ x, int64_t n, const float *__restrict__ params,
                                                             GridLevels lv, float *__restrict__ out)
{
    const int l = blockIdx.y;
    const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n) return;
    float p[3];
    load_point(x, i, p);
    const Cell cl = cell_of(p, lv.scale[l]);
    const uint32_t res = lv.res[l], entries = lv.entries[l];
    const bool hashed = lv.hashed[l] != 0;
    const float *table = params + lv.offset[l] * F;
    float acc[F];
#pragma unroll
    for (int f = 0; f < F; ++f) acc[f] = 0.0f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        float v[F];
        load_feat<F>(table + int64_t(corner_index(cl, c, res, entries, hashed)) * F, v);
        const float w = corner_weight(cl, c);
#pragma unroll
        for (int f = 0; f < F; ++f) acc[f] = fmaf(w, v[f], acc[f]);
    }
    store_feat<F>(out + i * (int64_t(lv.n_levels) * F) + int64_t(l) * F, acc);
}

template <int F>
__global__ __launch_bounds__(kBlock) void grid_backward_params_kernel(const float *__restrict__ x, int64_t n, GridLevels lv,
                                                                      const float *__restrict__ grad_out, float *__restrict__ grad_params)
{
    const int l = lv.lds_levels + blockIdx.y;
    const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    const bool valid = i < n;                       // no early return: the whole wave takes part in combine_runs
    float p[3] = {0.0f, 0.0f, 0.0f}, g[F];
#pragma unroll
    for (int f = 0; f < F; ++f) g[f] = 0.0f;
    if (valid) {
        load_point(x, i, p);
        load_feat<F>(grad_out + i * (int64_t(lv.n_levels) * F) + int64_t(l) * F, g);
    }
    const Cell cl = cell_of(p, lv.scale[l]);
    const uint32_t res = lv.res[l], entries = lv.entries[l];
    const bool hashed = lv.hashed[l] != 0;
    float *table = grad_params + lv.offset[l] * F;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const uint32_t key = valid ? corner_index(cl, c, res, entries, hashed) : kInvalid;
        const float w = corner_weight(cl, c);
        float v[F];
#pragma unroll
        for (int f = 0; f < F; ++f) v[f] = w * g[f];
        if (combine_runs<F>(key, v) && valid) {
            float *dst = table + int64_t(key) * F;
#pragma unroll
            for (int f = 0; f < F; ++f) atomicAdd(dst + f, v[f]);
        }
    }
}

template <int F>
__global__ __launch_bounds__(kLdsBlock) void grid_backward_params_lds_kernel(const float *__restrict__ x, int64_t n, GridLevels lv, int l,
                                                                             const float *__restrict__ grad_out,
                                                                             float *__restrict__ grad_params)
{
    extern __shared__ float acc[];
    const uint32_t n_floats = lv.entries[l] * F;
    for (uint32_t j = threadIdx.x; j < n_floats; j += kLdsBlock) acc[j] = 0.0f;
    __syncthreads();
    const float scale = lv.scale[l];
    const uint32_t res = lv.res[l], entries = lv.entries[l];
    const bool hashed = lv.hashed[l] != 0;
    const int64_t row = int64_t(lv.n_levels) * F;
    const int64_t stride = int64_t(gridDim.x) * kLdsBlock;
    // the loop bound is the same for the whole wave (n rounded up to the stride's multiple of 64): combine_runs needs every lane
    const int64_t n_wave = (n + 63) & ~int64_t(63);
    for (int64_t i = int64_t(blockIdx.x) * kLdsBlock + threadIdx.x; i < n_wave; i += stride) {
        const bool valid = i < n;
        float p[3] = {0.0f, 0.0f, 0.0f}, g[F];
#pragma unroll
        for (int f = 0; f < F; ++f) g[f] = 0.0f;
        if (valid) {
            load_point(x, i, p);
            load_feat<F>(grad_out + i * row + int64_t(l) * F, g);
        }
        const Cell cl = cell_of(p, scale);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const uint32_t key = valid ? corner_index(cl, c, res, entries, hashed) : kInvalid;
            const float w = corner_weight(cl, c);
            float v[F];
#pragma unroll
            for (int f = 0; f < F; ++f) v[f] = w * g[f];
            if (combine_runs<F>(key, v) && valid) {
#pragma unroll
                for (int f = 0; f < F; ++f) atomicAdd(&acc[key * F + f], v[f]);
            }
        }
    }
    __syncthreads();
    float *dst = grad_params + lv.offset[l] * F;
    for (uint32_t j = threadIdx.x; j < n_floats; j += kLdsBlock) {
        const float v = acc[j];
        if (v != 0.0f) atomicAdd(dst + j, v);
    }
}

template <int F>
__global__ __launch_bounds__(kBlock) void grid_backward_x_kernel(const float *__restrict__ x, int64_t n, const float *__restrict__ params,
                                                                 GridLevels lv, const float *__restrict__ grad_out, float *__restrict__ grad_x)
{
    const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n) return;
    float p[3];
    load_point(x, i, p);
    const float *grow = grad_out + i * (int64_t(lv.n_levels) * F);
    float gx[3] = {0.0f, 0.0f, 0.0f};
    for (int l = 0; l < lv.n_levels; ++l) {
        float g[F];
        load_feat<F>(grow + l * F, g);
        const Cell cl = cell_of(p, lv.scale[l]);
        const uint32_t res = lv.res[l], entries = lv.entries[l];
        const bool hashed = lv.hashed[l] != 0;
        const float *table = params + lv.offset[l] * F;
        float gl[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            float v[F];
            load_feat<F>(table + int64_t(corner_index(cl, c, res, entries, hashed)) * F, v);
            float s = 0.0f;                                       // dL / d(corner weight)
#pragma unroll
            for (int f = 0; f < F; ++f) s = fmaf(v[f], g[f], s);
            const float wx = (c & 1) ? cl.f[0] : 1.0f - cl.f[0];
            const float wy = (c & 2) ? cl.f[1] : 1.0f - cl.f[1];
            const float wz = (c & 4) ? cl.f[2] : 1.0f - cl.f[2];
            gl[0] += ((c & 1) ? s : -s) * wy * wz;
            gl[1] += ((c & 2) ? s : -s) * wx * wz;
            gl[2] += ((c & 4) ? s : -s) * wx * wy;
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) gx[d] = fmaf(gl[d], lv.scale[l], gx[d]);
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) grad_x[3 * i + d] = gx[d];
}

inline unsigned blocks_of(int64_t n) { return unsigned((n + kBlock - 1) / kBlock); }

template <int F>
hipError_t encode_f(const float *x, int64_t n, const float *params, const GridLevels &lv, float *out, hipStream_t stream)
{
    hipLaunchKernelGGL(grid_encode_kernel<F>, dim3(blocks_of(n), lv.n_levels), dim3(kBlock), 0, stream, x, n, params, lv, out);
    return hipGetLastError();
}

template <int F>
hipError_t backward_f(const float *x, int64_t n, const float *params, const GridLevels &lv, const float *grad_out, float *grad_params,
                      float *grad_x, hipStream_t stream)
{
    if (grad_params) {
        for (int l = 0; l < lv.lds_levels; ++l) {
            const int bytes = int(lv.entries[l]) * F * int(sizeof(float));
            if (bytes > 64 * 1024) {                     // (per function and device; always raised to the same cap)
                hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&grid_backward_params_lds_kernel<F>),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, kGridLdsBytes);
                if (e != hipSuccess) return e;
            }
            // about 16 points per lane and at most one workgroup per CU: the table flush stays small against the points
            const int64_t want = (n + int64_t(kLdsBlock) * 16 - 1) / (int64_t(kLdsBlock) * 16);
            const unsigned nblk = unsigned(want < 1 ? 1 : (want > 256 ? 256 : want));
            hipLaunchKernelGGL(grid_backward_params_lds_kernel<F>, dim3(nblk), dim3(kLdsBlock), bytes, stream, x, n, lv, l, grad_out,
                               grad_params);
            hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
        if (lv.n_levels > lv.lds_levels) {
            hipLaunchKernelGGL(grid_backward_params_kernel<F>, dim3(blocks_of(n), lv.n_levels - lv.lds_levels), dim3(kBlock), 0, stream, x,
                               n, lv, grad_out, grad_params);
            hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
    }
    if (grad_x) {
        hipLaunchKernelGGL(grid_backward_x_kernel<F>, dim3(blocks_of(n)), dim3(kBlock), 0, stream, x, n, params, lv, grad_out, grad_x);
        return hipGetLastError();
    }
    return hipSuccess;
}

}  // namespace

hipError_t launch_grid_encode(const float *x, int64_t n, const float *params, const GridLevels &lv, int32_t n_features, float *out,
                              hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    switch (n_features) {
    case 1: return encode_f<1>(x, n, params, lv, out, stream);
    case 2: return encode_f<2>(x, n, params, lv, out, stream);
    case 4: return encode_f<4>(x, n, params, lv, out, stream);
    case 8: return encode_f<8>(x, n, params, lv, out, stream);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_grid_encode_backward(const float *x, int64_t n, const float *params, const GridLevels &lv, int32_t n_features,
                                       const float *grad_out, float *grad_params, float *grad_x, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    switch (n_features) {
    case 1: return backward_f<1>(x, n, params, lv, grad_out, grad_params, grad_x, stream);
    case 2: return backward_f<2>(x, n, params, lv, grad_out, grad_params, grad_x, stream);
    case 4: return backward_f<4>(x, n, params, lv, grad_out, grad_params, grad_x, stream);
    case 8: return backward_f<8>(x, n, params, lv, grad_out, grad_params, grad_x, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace tsamd
