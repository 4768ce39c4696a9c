// gfx950 (MI355X / CDNA4) streaming kernels around the tile kernel (tile_kernel.hip): what ends an evaluation -- the finish
// kernel, the energy reduction -- and what follows it in an optimisation step -- gradient scaling and limiting, AdamUniform.
// The launch layer (eval_launch.cpp) reaches the first group through step_kernels(); the rest have their launchers here.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "launch_args.h"

namespace tsamd {
namespace {

constexpr int kWave = 64;

// Per-tile energy partials -> E = c1 E_s + c2 E_b (tet_spheres_cuda.cu:191), one workgroup of T threads, fixed
// order (bitwise repeatable).  Each thread owns tiles tid, tid + T, ... and issues its loads in batches of eight
// before summing: a plain dependent loop costs one HBM latency per tile (60 us for 19 k tiles).
template <int T>
__device__ __forceinline__ void energy_reduce(const FinishArgs &a, double *red)
{
    const int tid = threadIdx.x;
    const double2 *part = reinterpret_cast<const double2 *>(a.partials);
    double s = 0.0, b = 0.0;
    int64_t t = tid;
    for (; t + 7 * T < a.n_tiles; t += 8 * T) {
        double2 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = part[t + u * T];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            s += v[u].x;
            b += v[u].y;
        }
    }
    for (; t < a.n_tiles; t += T) {
        const double2 v = part[t];
        s += v.x;
        b += v.y;
    }
    red[tid] = s;
    red[T + tid] = b;
    __syncthreads();
    for (int off = T / 2; off > 0; off >>= 1) {
        if (tid < off) {
            red[tid] += red[tid + off];
            red[T + tid] += red[T + tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) {
        a.terms[0] = red[0];
        a.terms[1] = red[T];
        const float c1 = a.coef ? a.coef[0] : a.c1, c2 = a.coef ? a.coef[1] : a.c2;
        const float e = float(double(c1) * red[0] + double(c2) * red[T]);
        a.energy[0] = e;
        if (a.energy_copy) a.energy_copy[0] = e;
    }
}

// Forward-only evaluations: just the energy.
__global__ __launch_bounds__(1024) void energy_reduce_kernel(const FinishArgs a)
{
    __shared__ double red[2 * 1024];
    energy_reduce<1024>(a, red);
}

// Workgroup 0 reduces the energy partials (when asked to) while the others sum, for every vertex touched by
// several tiles, its staged partial gradients in plan order (deterministic): one launch, and the 8 us of the
// single-workgroup reduction hide behind the vertex work.
// (Ordinary loads: non-temporal ones for the staging rows and lists -- read for the last time / once per evaluation -- were measured,
// round 6: finish kernel 0.0269 -> 0.0409 ms on 512 x kuhn19, 0.0297 -> 0.0414 on a.veg x 952.  The rows are still in the memory-side
// cache from the tile kernel's stores; a non-temporal read gives that up.)
#define FIN_LOAD(p) (*(p))
// One finish vertex: grad[vid] = gscale * (sum of staging rows [e0, e1), in order).
__device__ __forceinline__ void finish_vertex(const FinishArgs &a, int32_t e0, int32_t e1, int32_t vid, float gscale)
{
    float gx = 0.f, gy = 0.f, gz = 0.f;
    // the first four rows go out together (most shared vertices have 2-4 copies): one memory latency instead of one
    // per row; rows beyond the vertex's own are re-reads of its last row and are not added.  Finish kernel 0.037 ->
    // 0.031 ms on the 512-sphere scene (2 / 3 / 8 rows: 0.034 / 0.031 / 0.031); same order of additions.
    constexpr int kRowsAhead = 4;
    {
        float3 r[kRowsAhead];
#pragma unroll
        for (int j = 0; j < kRowsAhead; ++j) {
            // (a vertex no tet references is in the list with zero rows: e1 - 1 may be -1 -- read row 0, add nothing)
            const int32_t e = e0 + j < e1 ? e0 + j : (e1 > 0 ? e1 - 1 : 0);
            const float *p = a.stage + size_t(e) * 3;
            r[j] = make_float3(FIN_LOAD(p), FIN_LOAD(p + 1), FIN_LOAD(p + 2));
        }
#pragma unroll
        for (int j = 0; j < kRowsAhead; ++j)
            if (e0 + j < e1) {
                gx += r[j].x;
                gy += r[j].y;
                gz += r[j].z;
            }
    }
    for (int32_t e = e0 + kRowsAhead; e < e1; ++e) {
        const float *r = a.stage + size_t(e) * 3;
        gx += FIN_LOAD(r);
        gy += FIN_LOAD(r + 1);
        gz += FIN_LOAD(r + 2);
    }
    float *g = a.grad + size_t(vid) * 3;
    g[0] = gx * gscale;
    g[1] = gy * gscale;
    g[2] = gz * gscale;
}

__global__ __launch_bounds__(256) void finish_kernel(const FinishArgs a)
{
    __shared__ double red[2 * 256];
    const int tid = threadIdx.x;
    if (blockIdx.x == 0) {
        if (a.energy && blockIdx.y == 0) energy_reduce<256>(a, red);
        return;
    }
    const float gscale = a.grad_out ? *a.grad_out : 1.f;
    if (a.reg_k > 0) {
        // Regular batch (launch_args.h): the grid is (1 + template entries / 256) x (copies, at most 65 535).  The template's three
        // list entries are bytes every copy reads -- cache hits, not one HBM round trip per vertex in front of its rows -- and are
        // read once per thread; each copy's rows and vertex follow by adding its constants.
        const int64_t kk = int64_t(blockIdx.x - 1) * 256 + tid;
        if (kk >= a.reg_k) return;
        const int32_t e0 = FIN_LOAD(&a.fin_off[kk]), e1 = FIN_LOAD(&a.fin_off[kk + 1]), vid = FIN_LOAD(&a.fin_vid[kk]);
        for (int c = int(blockIdx.y); c < a.reg_copies; c += int(gridDim.y)) finish_vertex(a, e0 + c * a.reg_s, e1 + c * a.reg_s, vid + c * a.reg_v, gscale);
        return;
    }
    // one thread per shared vertex (measured faster than one thread per output float: 0.065 vs 0.093 ms)
    const int64_t stride = int64_t(gridDim.x - 1) * 256;
    for (int64_t k = int64_t(blockIdx.x - 1) * 256 + tid; k < a.n_finish; k += stride) {
        const int32_t e0 = FIN_LOAD(&a.fin_off[k]), e1 = FIN_LOAD(&a.fin_off[k + 1]);   // consecutive rows, tile order
        finish_vertex(a, e0, e1, FIN_LOAD(&a.fin_vid[k]), gscale);
    }
}

__global__ __launch_bounds__(256) void scale_kernel(const float *in, const float *scalar, float *out, int64_t n)
{
    const float s = *scalar;
    if (in == out && s == 1.f) return;  // in-place by exactly 1 (the usual autograd grad_output): nothing to do
    const int64_t stride = int64_t(gridDim.x) * 256;
    const int64_t n4 = n >> 2;
    const float4 *in4 = reinterpret_cast<const float4 *>(in);
    float4 *out4 = reinterpret_cast<float4 *>(out);
    const bool vec = ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    if (vec) {
        for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n4; i += stride) {
            float4 v = in4[i];
            out4[i] = make_float4(v.x * s, v.y * s, v.z * s, v.w * s);
        }
        for (int64_t i = 4 * n4 + int64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += stride) out[i] = in[i] * s;
    } else {
        for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += stride) out[i] = in[i] * s;
    }
}

// max |g| over the array, as the bit pattern of a non-negative float (monotone under uint compare)
__global__ __launch_bounds__(256) void absmax_kernel(const float *g, int64_t n, unsigned int *out)
{
    __shared__ float red[256 / kWave];
    float m = 0.f;
    const int64_t stride = int64_t(gridDim.x) * 256;
    for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += stride) m = fmaxf(m, fabsf(g[i]));
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) m = fmaxf(m, __shfl_down(m, off, kWave));
    if (threadIdx.x % kWave == 0) red[threadIdx.x / kWave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 256 / kWave; ++w) m = fmaxf(m, red[w]);
        atomicMax(out, __float_as_uint(m));
    }
}

__global__ __launch_bounds__(256) void clamp_kernel(float *g, int64_t n, const unsigned int *mx, float thr, float s)
{
    const float m = __uint_as_float(*mx);
    if (!(m > thr)) return;
    const float f = s / m;
    const int64_t stride = int64_t(gridDim.x) * 256;
    for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += stride) g[i] *= f;
}

// ---- AdamUniform (reference utils/optimizer.py:38-89), two passes, no host sync ----
// pass 1: moments in place (optimizer.py:61-62) + max g2 and max |g1| (the two global maxima the reference
//         takes with .max(), :74 and :84, are monotone in the bias-corrected values)
__global__ __launch_bounds__(256) void adam_moments_kernel(const float *grad, float *g1, float *g2, int64_t n, float b1,
                                                           float b2, unsigned int *ws)
{
    __shared__ float red[2 * (256 / kWave)];
    float mx2 = 0.f, mx1 = 0.f;
    const int64_t stride = int64_t(gridDim.x) * 256, gid = int64_t(blockIdx.x) * 256 + threadIdx.x;
    auto upd = [&](float g, float &a, float &b) {
        a = a * b1 + g * (1.f - b1);
        b = b * b2 + (g * g) * (1.f - b2);
        mx1 = fmaxf(mx1, fabsf(a));
        mx2 = fmaxf(mx2, b);
    };
    // 16 B per lane (torch allocations are 16-B aligned; the tail and odd alignments take the scalar loop)
    const bool vec = ((reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(g1) | reinterpret_cast<uintptr_t>(g2)) & 15) == 0;
    const int64_t n4 = vec ? n >> 2 : 0;
    for (int64_t i = gid; i < n4; i += stride) {
        const float4 g = reinterpret_cast<const float4 *>(grad)[i];
        float4 a = reinterpret_cast<float4 *>(g1)[i], b = reinterpret_cast<float4 *>(g2)[i];
        upd(g.x, a.x, b.x);
        upd(g.y, a.y, b.y);
        upd(g.z, a.z, b.z);
        upd(g.w, a.w, b.w);
        reinterpret_cast<float4 *>(g1)[i] = a;
        reinterpret_cast<float4 *>(g2)[i] = b;
    }
    for (int64_t i = 4 * n4 + gid; i < n; i += stride) {
        float a = g1[i], b = g2[i];
        upd(grad[i], a, b);
        g1[i] = a;
        g2[i] = b;
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        mx1 = fmaxf(mx1, __shfl_down(mx1, off, kWave));
        mx2 = fmaxf(mx2, __shfl_down(mx2, off, kWave));
    }
    const int wave = threadIdx.x / kWave;
    if (threadIdx.x % kWave == 0) {
        red[2 * wave] = mx1;
        red[2 * wave + 1] = mx2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 256 / kWave; ++w) {
            mx1 = fmaxf(mx1, red[2 * w]);
            mx2 = fmaxf(mx2, red[2 * w + 1]);
        }
        atomicMax(ws, __float_as_uint(mx1));      // non-negative floats order like their bit patterns
        atomicMax(ws + 1, __float_as_uint(mx2));
    }
}

// pass 2: gr = m1 / (1e-8 + max sqrt(m2)) (:74), optional max-abs clamp to `limit` (:84-86), p -= lr * gr (:88)
__global__ __launch_bounds__(256) void adam_apply_kernel(float *p, const float *g1, int64_t n, float lr, float bias1,
                                                         float bias2, float limit, const unsigned int *ws)
{
    const float mx1 = __uint_as_float(ws[0]) / bias1;             // max |m1|
    const float denom = 1e-8f + sqrtf(__uint_as_float(ws[1]) / bias2);
    float scale = 1.f / denom;
    const float s = mx1 / denom;                                  // max |gr|
    if (limit > 0.f && s > limit) scale *= limit / s;
    const float k = lr * scale / bias1;
    const int64_t stride = int64_t(gridDim.x) * 256, gid = int64_t(blockIdx.x) * 256 + threadIdx.x;
    const bool vec = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g1)) & 15) == 0;
    const int64_t n4 = vec ? n >> 2 : 0;
    for (int64_t i = gid; i < n4; i += stride) {
        float4 v = reinterpret_cast<float4 *>(p)[i];
        const float4 a = reinterpret_cast<const float4 *>(g1)[i];
        v.x -= k * a.x;
        v.y -= k * a.y;
        v.z -= k * a.z;
        v.w -= k * a.w;
        reinterpret_cast<float4 *>(p)[i] = v;
    }
    for (int64_t i = 4 * n4 + gid; i < n; i += stride) p[i] -= k * g1[i];
}

// Grid of the kernels that end in one atomicMax per workgroup (adam_moments_kernel, absmax_kernel): few, long-running workgroups.
// The atomics of all workgroups hit the same two words and serialise: 4 096 workgroups cost AdamUniform.step 0.127 ms at 12.3 M
// elements, 512 cost 0.065 (6.0 TB/s algorithmic), 256 0.063, 16 384 0.305; 0.705 against 0.802 ms at 120 M elements.
constexpr int kReduceGridCap = 512;

int grid_for(int64_t n, int per_block, int cap)
{
    int64_t b = (n + per_block - 1) / per_block;
    return int(b < 1 ? 1 : (b > cap ? cap : b));
}

}  // namespace

StepKernels step_kernels()
{
    return {reinterpret_cast<const void *>(&finish_kernel), reinterpret_cast<const void *>(&energy_reduce_kernel),
            reinterpret_cast<const void *>(&adam_moments_kernel), reinterpret_cast<const void *>(&adam_apply_kernel)};
}

// workgroup 0 for the energy + one vertex per thread: the per-vertex chain off[k] -> rows -> store is pure latency, so expose all of it
unsigned finish_grid(int64_t n_finish) { return 1u + unsigned(grid_for(n_finish, 256, 1 << 20)); }
// regular batch: x as above over the entries of ONE copy, y over the copies (a thread walks copies y, y + grid.y, ...)
dim3 finish_grid_regular(int64_t per_copy, int copies) { return dim3(finish_grid(per_copy), unsigned(copies < 65535 ? copies : 65535)); }

unsigned adam_grid(int64_t n) { return unsigned(grid_for(n, 1024, kReduceGridCap)); }

hipError_t launch_scale(const float *in, const float *scalar, float *out, int64_t n, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(scale_kernel, dim3(unsigned(grid_for(n, 1024, 2048))), dim3(256), 0, stream, in, scalar, out, n);
    return hipGetLastError();
}

hipError_t launch_adam_uniform(float *p, const float *grad, float *g1, float *g2, int64_t n, float lr, float b1, float b2,
                               float bias1, float bias2, float limit, void *workspace, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    unsigned int *ws = static_cast<unsigned int *>(workspace);
    hipError_t e = hipMemsetAsync(ws, 0, 2 * sizeof(unsigned int), stream);
    if (e != hipSuccess) return e;
    const int g = grid_for(n, 1024, kReduceGridCap);
    hipLaunchKernelGGL(adam_moments_kernel, dim3(unsigned(g)), dim3(256), 0, stream, grad, g1, g2, n, b1, b2, ws);
    hipLaunchKernelGGL(adam_apply_kernel, dim3(unsigned(g)), dim3(256), 0, stream, p, g1, n, lr, bias1, bias2, limit, ws);
    return hipGetLastError();
}

hipError_t launch_grad_limit(float *grad, int64_t n, float thr, float s, void *workspace, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    unsigned int *mx = static_cast<unsigned int *>(workspace);
    hipError_t e = hipMemsetAsync(mx, 0, sizeof(unsigned int), stream);
    if (e != hipSuccess) return e;
    const int g = grid_for(n, 1024, kReduceGridCap);
    hipLaunchKernelGGL(absmax_kernel, dim3(unsigned(g)), dim3(256), 0, stream, grad, n, mx);
    hipLaunchKernelGGL(clamp_kernel, dim3(unsigned(g)), dim3(256), 0, stream, grad, n, mx, thr, s);
    return hipGetLastError();
}

}  // namespace tsamd
