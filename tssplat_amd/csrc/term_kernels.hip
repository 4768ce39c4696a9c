// gfx950 kernels of the renderer slice: the id-driven image terms -- masked MSE (det_mean.h) of a value of the interpolated vertex
// attribute and both of its scatters, without an image chain, from the ids of the alpha stage (raster_kernels.hip: silhouette_cover_kernel).
// A term takes a value x[kChannels] of the point y = interpolate(attr, rast) of a [V, 3] vertex attribute; its loss is the mean over
// pixels and channels of (x_c m - t_c m)^2, the mask broadcast over the channels.  The depth term is what the reference's
// trainer.py:104-115 builds from out["d"] = ||interpolate(v_pos, rast) - campos|| (mesh_rasterizer.py:151-161); the normal term what
// MeshRasterizer.forward(fit_normal=True) and a masked MSELoss build from out["n"] = interpolate(attr, rast) (mesh_rasterizer.py:137-149;
// `attr` is any [V, 3] attribute: the normal is the use).  Per pixel those chains move a 16-byte rast pixel, a 12-byte interpolated
// pixel, the masked products and their gradients; here a pixel is its triangle id (the alpha stage's by-product), kChannels target floats
// and a mask -- 12 or 20 bytes -- plus cached vertex gathers.  (u, v) are the clamped barycentrics of the resolve pass (edge_functions,
// the same operations), w = 1 - u - v and the interpolation are interpolate_kernel's; a background pixel has y = 0, so d = ||campos||
// and n = 0, as in the chains.
#include <hip/hip_runtime.h>

#include "det_mean.h"
#include "raster.h"
#include "raster_device.h"

namespace tsamd {
namespace {

// A term is the only place that knows "distance to a camera" from "the attribute itself": its channel count, its per-view constants,
// its value x at the interpolated point y of a view, and the pull-back of dL/dx to g = dL/dy.  The operations and their order are the
// result's bits (this file is compiled without contraction).
struct DepthTerm {
    static constexpr int kChannels = 1;
    const float *campos;   // [batch, 3]

    __device__ __forceinline__ void value(int64_t view, const float y[3], float x[1]) const
    {
        const float *c = campos + 3 * view;
        const float dx = y[0] - c[0], dy = y[1] - c[1], dz = y[2] - c[2];
        x[0] = sqrtf(dx * dx + dy * dy + dz * dz);
    }
    // d = ||y - c||: g = g_d (y - c) / d, 0 where d = 0
    __device__ __forceinline__ void pull(int64_t view, const float y[3], const float x[1], const float gx[1], float g[3]) const
    {
        const float *c = campos + 3 * view;
#pragma unroll
        for (int k = 0; k < 3; ++k) g[k] = x[0] == 0.f ? 0.f : gx[0] * ((y[k] - c[k]) / x[0]);
    }
};

struct NormalTerm {
    static constexpr int kChannels = 3;

    __device__ __forceinline__ void value(int64_t, const float y[3], float x[3]) const { x[0] = y[0], x[1] = y[1], x[2] = y[2]; }
    __device__ __forceinline__ void pull(int64_t, const float *, const float *, const float gx[3], float g[3]) const { g[0] = gx[0], g[1] = gx[1], g[2] = gx[2]; }
};

constexpr int kTermPixels = 4;                                  // 64-pixel chunks per wave and round, all their loads in flight together
constexpr int kTermPerBlock = kMeanBlock * kTermPixels;         // pixels per workgroup and round
constexpr int kTermMaxBlocks = 8192;                            // (the loss's bits depend on these two: det_mean.h)

// One lane per pixel; a workgroup strides over rounds of kTermPerBlock pixels and stores one double: the sum over its pixels and the
// term's channels of (x_c m - t_c m)^2, each product rounded on its own, squared and added in float64 (channel 0, 1, .. in turn).
// x_out (optional): the term's image [B, H, W, kChannels], every pixel of it.
template <class Term>
__global__ __launch_bounds__(kMeanBlock) void term_mse_kernel(const float4 *pos, const int32_t *tri, int64_t n_vertices, int64_t n_tri, int64_t batch, int height,
                                                              int width, const int32_t *ids, const float *attr, Term term, const float *target, const float *mask,
                                                              double *partials, float *x_out)
{
    constexpr int K = kTermPixels, C = Term::kChannels;
    __shared__ double lds[kMeanBlock / 64];
    const int64_t hw = int64_t(height) * width, total = batch * hw;
    const int lane = int(threadIdx.x) & 63, wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
    double acc = 0.0;
    for (int64_t first = int64_t(blockIdx.x) * kTermPerBlock; first < total; first += int64_t(gridDim.x) * kTermPerBlock) {
        const int64_t gid0 = first + int64_t(wave) * (64 * K);
        int32_t id[K];
        float tg[K][C], m[K];
        bool want[K];
        // all global loads first, together (the latency of one round trip, not of three)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int64_t gid = gid0 + 64 * k + lane;
            const bool have = gid < total;
            id[k] = have ? ids[gid] : 0;
            m[k] = have ? mask[gid] : 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) tg[k][c] = have ? target[C * gid + c] : 0.f;
            want[k] = have && (m[k] != 0.f || x_out != nullptr);     // a masked-out pixel adds 0: no vertex work unless its x is asked for
        }
        bool any = false;
#pragma unroll
        for (int k = 0; k < K; ++k) any = any || want[k];
        if (__ballot(any) == 0ull) continue;                          // wave-uniform: nothing in these chunks enters the loss
        const WavePixels<K> p = wave_pixels<K>(gid0, lane, total, hw, width);   // (behind the loads and the test: a scalar 64-bit division)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (!want[k]) continue;
            float y[3] = {0.f, 0.f, 0.f}, x[C];
            int32_t i0, i1, i2;
            if (triangle_of_id(id[k], tri, n_tri, n_vertices, i0, i1, i2)) {
                float u, v, w, a[9];
                weights_and_gather(pos + p.b[k] * n_vertices, attr, i0, i1, i2, p.px[k], p.py[k], height, width, u, v, w, a);
#pragma unroll
                for (int c = 0; c < 3; ++c) y[c] = u * a[c] + v * a[3 + c] + w * a[6 + c];
            }
            term.value(p.b[k], y, x);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                if (x_out) x_out[C * p.gid[k] + c] = x[c];
                const float r = x[c] * m[k] - tg[k][c] * m[k];
                acc += double(r) * double(r);
            }
        }
    }
    const double sum = block_sum(acc, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}

// One lane per pixel, one pass: (u, v, y, x) recomputed, g_c = grad_loss 2 (x_c m - t_c m) m / (kChannels pixels) pulled back to g = dL/dy,
// then BOTH scatters behind one run detection -- interpolate_backward's (u, v, w) g into grad_attr[V, 3] and, through
// (du, dv) = (g . (a0 - a2), g . (a1 - a2)) and the quotient rule of rasterize_backward, (x, y, w) into grad_pos[B, V, 4].
// The run key holds the view: grad_pos is per view, and a wave of a small image spans several views that show the same triangle.
// No gradient image and no grad_rast exist; background and masked-out pixels add nothing.  EVERY lane reaches find_runs.
template <class Term>
__global__ __launch_bounds__(256) void term_mse_backward_kernel(const float4 *pos, const int32_t *tri, int64_t n_vertices, int64_t n_tri, int64_t batch, int height,
                                                                int width, const int32_t *ids, const float *attr, Term term, const float *target,
                                                                const float *mask, const float *grad_loss, float *grad_attr, float4 *grad_pos)
{
    constexpr int C = Term::kChannels;
    const int64_t gid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const int64_t hw = int64_t(height) * width, total = batch * hw;
    bool valid = gid < total;
    int32_t id = 0, i0 = 0, i1 = 0, i2 = 0;
    float tg[C] = {}, m = 0.f;
    if (valid) {
        id = ids[gid], m = mask[gid];
#pragma unroll
        for (int c = 0; c < C; ++c) tg[c] = target[C * gid + c];
    }
    valid = valid && m != 0.f && triangle_of_id(id, tri, n_tri, n_vertices, i0, i1, i2);   // (background: y = 0 is a constant)
    int64_t b = 0;
    float da[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // the three channels of the three attribute rows
    float dc[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // (x, y, w) of the three clip-space positions
    if (valid) {
        int px, py;
        locate_pixel(gid, hw, width, false, 0, b, px, py);
        float u, v, w, a[9], y[3], x[C], gx[C], g[3];
        const EdgeFunctions e = weights_and_gather(pos + b * n_vertices, attr, i0, i1, i2, px, py, height, width, u, v, w, a);
#pragma unroll
        for (int c = 0; c < 3; ++c) y[c] = u * a[c] + v * a[3 + c] + w * a[6 + c];
        term.value(b, y, x);
        const float scale = grad_loss[0] / float(C * total);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float r = x[c] * m - tg[c] * m;
            gx[c] = (2.f * r * m) * scale;
        }
        term.pull(b, y, x, gx, g);
#pragma unroll
        for (int c = 0; c < 3; ++c) da[c] = u * g[c], da[3 + c] = v * g[c], da[6 + c] = w * g[c];
        const float du = g[0] * (a[0] - a[6]) + g[1] * (a[1] - a[7]) + g[2] * (a[2] - a[8]);
        const float dv = g[0] * (a[3] - a[6]) + g[1] * (a[4] - a[7]) + g[2] * (a[5] - a[8]);
        edge_functions_backward(e, du, dv, dc);
    }
    const Runs runs = find_runs(valid ? b * (int64_t(1) << 32) + int64_t(id) : -1 - int64_t(threadIdx.x));
#pragma unroll
    for (int k = 0; k < 9; ++k) da[k] = run_sum(runs, da[k]), dc[k] = run_sum(runs, dc[k]);
    if (valid && runs.last) {
        float *gp = reinterpret_cast<float *>(grad_pos + b * n_vertices);
        const int64_t at[3] = {int64_t(i0), int64_t(i1), int64_t(i2)};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            atomicAdd(grad_attr + 3 * at[k] + 0, da[3 * k]);
            atomicAdd(grad_attr + 3 * at[k] + 1, da[3 * k + 1]);
            atomicAdd(grad_attr + 3 * at[k] + 2, da[3 * k + 2]);
            atomicAdd(gp + 4 * at[k] + 0, dc[3 * k]);
            atomicAdd(gp + 4 * at[k] + 1, dc[3 * k + 1]);
            atomicAdd(gp + 4 * at[k] + 3, dc[3 * k + 2]);
        }
    }
}

template <class Term>
hipError_t launch_term_mse(const float *pos_clip, int64_t batch, int64_t n_vertices, const int32_t *tri, int64_t n_tri, int height, int width, const int32_t *ids,
                           const float *attr, Term term, const float *target, const float *mask, void *workspace, float *loss, float *x_out, hipStream_t stream)
{
    const int64_t pixels = pixel_count(batch, height, width);
    if (pixels <= 0 || n_tri <= 0) return hipMemsetAsync(loss, 0, sizeof(float), stream);
    const int blocks = mean_blocks(pixels, kTermPerBlock, kTermMaxBlocks);
    hipLaunchKernelGGL(term_mse_kernel<Term>, dim3(blocks), dim3(kMeanBlock), 0, stream, reinterpret_cast<const float4 *>(pos_clip), tri, n_vertices, n_tri, batch,
                       height, width, ids, attr, term, target, mask, static_cast<double *>(workspace), x_out);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : launch_mean_final(workspace, blocks, Term::kChannels * pixels, loss, stream);
}

template <class Term>
hipError_t launch_term_mse_backward(const float *pos_clip, int64_t batch, int64_t n_vertices, const int32_t *tri, int64_t n_tri, int height, int width,
                                    const int32_t *ids, const float *attr, Term term, const float *target, const float *mask, const float *grad_loss,
                                    int accumulate_pos, float *grad_attr, float *grad_pos, hipStream_t stream)
{
    hipError_t e;
    if (n_vertices > 0 && (e = hipMemsetAsync(grad_attr, 0, size_t(n_vertices) * 3 * sizeof(float), stream)) != hipSuccess) return e;
    if (!accumulate_pos && batch * n_vertices > 0 &&
        (e = hipMemsetAsync(grad_pos, 0, size_t(batch) * size_t(n_vertices) * 4 * sizeof(float), stream)) != hipSuccess)
        return e;
    const int64_t pixels = pixel_count(batch, height, width);
    if (pixels <= 0 || n_tri <= 0 || n_vertices <= 0) return hipSuccess;
    hipLaunchKernelGGL(term_mse_backward_kernel<Term>, dim3(unsigned((pixels + 255) / 256)), dim3(256), 0, stream, reinterpret_cast<const float4 *>(pos_clip), tri, n_vertices,
                       n_tri, batch, height, width, ids, attr, term, target, mask, grad_loss, grad_attr, reinterpret_cast<float4 *>(grad_pos));
    return hipGetLastError();
}

}  // namespace

int64_t depth_mse_workspace_bytes(int64_t n) { return mean_workspace_bytes(mean_blocks(n, kTermPerBlock, kTermMaxBlocks)); }
int64_t normal_mse_workspace_bytes(int64_t n) { return depth_mse_workspace_bytes(n); }

hipError_t launch_depth_mse(const float *pos_clip, int64_t batch, int64_t n_vertices, const int32_t *tri, int64_t n_tri, int height, int width, const int32_t *ids,
                            const float *world_pos, const float *campos, const float *target, const float *mask, void *workspace, float *loss, float *depth_out,
                            hipStream_t stream)
{
    return launch_term_mse(pos_clip, batch, n_vertices, tri, n_tri, height, width, ids, world_pos, DepthTerm{campos}, target, mask, workspace, loss, depth_out, stream);
}

hipError_t launch_depth_mse_backward(const float *pos_clip, int64_t batch, int64_t n_vertices, const int32_t *tri, int64_t n_tri, int height, int width,
                                     const int32_t *ids, const float *world_pos, const float *campos, const float *target, const float *mask, const float *grad_loss,
                                     int accumulate_pos, float *grad_world, float *grad_pos, hipStream_t stream)
{
    return launch_term_mse_backward(pos_clip, batch, n_vertices, tri, n_tri, height, width, ids, world_pos, DepthTerm{campos}, target, mask, grad_loss, accumulate_pos,
                                    grad_world, grad_pos, stream);
}

hipError_t launch_normal_mse(const float *pos_clip, int64_t batch, int64_t n_vertices, const int32_t *tri, int64_t n_tri, int height, int width, const int32_t *ids,
                             const float *attr, const float *target, const float *mask, void *workspace, float *loss, float *normal_out, hipStream_t stream)
{
    return launch_term_mse(pos_clip, batch, n_vertices, tri, n_tri, height, width, ids, attr, NormalTerm{}, target, mask, workspace, loss, normal_out, stream);
}

hipError_t launch_normal_mse_backward(const float *pos_clip, int64_t batch, int64_t n_vertices, const int32_t *tri, int64_t n_tri, int height, int width,
                                      const int32_t *ids, const float *attr, const float *target, const float *mask, const float *grad_loss, int accumulate_pos,
                                      float *grad_attr, float *grad_pos, hipStream_t stream)
{
    return launch_term_mse_backward(pos_clip, batch, n_vertices, tri, n_tri, height, width, ids, attr, NormalTerm{}, target, mask, grad_loss, accumulate_pos, grad_attr,
                                    grad_pos, stream);
}

}  // namespace tsamd
