// gfx950 kernels of the texture side of the renderer slice: the per-triangle atlas bake and dr.texture.
//   atlas_bake_kernel                       one lane per texel: owner and barycentrics in closed form from (i, j), no table
//   texture_nearest_kernel / _linear_kernel one lane per output pixel, loop over the channels
//   texture_*_backward_kernel               the same lanes: dL/dtex by fp32 global atomics (hardware adds, not a
//                                           compare-and-swap loop; the order of the adds, and so the last bits, vary from run
//                                           to run), dL/duv per pixel from the taps actually used
// Semantics: tests/atlas_oracle.py, tests/texture_oracle.py.  Built with -ffp-contract=off (_build.py): x = u W - 0.5 is a
// rounded product and then an exact or rounded difference, as the oracle states it, not one fused operation.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "texture.h"

namespace tsamd {

namespace {

constexpr int kBlock = 256;

unsigned blocks_for(int64_t n) { return unsigned((n + kBlock - 1) / kBlock); }

// Texel (i, j) of an R x R atlas: column i, row j, centre (i + 0.5, j + 0.5).  Cell k = (j / c) n + i / c holds triangle 2 k
// (half A, local i + j <= L + 3) and 2 k + 1 (half B, local i + j >= 2 c - L - 5); the diagonal band between them, the texels
// outside the n c square and the halves of triangles >= T are unowned.  Barycentrics are extrapolated into the gutter:
// A: b1 = (i - 1) / L, b2 = (j - 1) / L; B: b1 = (c - 2 - i) / L, b2 = (c - 2 - j) / L; b0 = 1 - b1 - b2.
__global__ __launch_bounds__(kBlock) void atlas_bake_kernel(const float *v_pos, int64_t n_vertices, const int32_t *tri, int64_t n_tri, int32_t res,
                                                            AtlasLayout lay, float *positions, int32_t *owner)
{
    const int64_t gid = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (gid >= int64_t(res) * res) return;
    const int32_t j = int32_t(gid / res), i = int32_t(gid - int64_t(j) * res);
    const int32_t n = lay.cells_per_row, c = lay.cell, L = lay.leg;
    const int32_t cx = i / c, cy = j / c;
    int64_t t = -1;
    float b1 = 0.f, b2 = 0.f;
    if (cx < n && cy < n) {
        const int32_t li = i - cx * c, lj = j - cy * c;
        const int64_t k = int64_t(cy) * n + cx;
        if (li + lj <= L + 3) {
            t = 2 * k;
            b1 = float(li - 1) / float(L), b2 = float(lj - 1) / float(L);
        } else if (li + lj >= 2 * c - L - 5) {
            t = 2 * k + 1;
            b1 = float(c - 2 - li) / float(L), b2 = float(c - 2 - lj) / float(L);
        }
    }
    float px = 0.f, py = 0.f, pz = 0.f;
    if (t >= n_tri) t = -1;
    if (t >= 0) {
        const int32_t i0 = tri[3 * t], i1 = tri[3 * t + 1], i2 = tri[3 * t + 2];
        // a triangle with a vertex index outside the position array is unowned (the rule of interpolate_kernel)
        if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= n_vertices || i1 >= n_vertices || i2 >= n_vertices) {
            t = -1;
        } else {
            const float *p0 = v_pos + int64_t(i0) * 3, *p1 = v_pos + int64_t(i1) * 3, *p2 = v_pos + int64_t(i2) * 3;
            const float b0 = 1.f - b1 - b2;
            px = b0 * p0[0] + b1 * p1[0] + b2 * p2[0];
            py = b0 * p0[1] + b1 * p1[1] + b2 * p2[1];
            pz = b0 * p0[2] + b1 * p1[2] + b2 * p2[2];
        }
    }
    float *o = positions + gid * 3;
    o[0] = px, o[1] = py, o[2] = pz;
    owner[gid] = int32_t(t);
}

enum { kWrap = 0, kClamp = 1, kZero = 2 };

// floor(x) as an index: kept within +-1e9 (and finite) so that index + 1 and the modulo below cannot overflow
__device__ __forceinline__ int floor_index(float x) { return int(fminf(fmaxf(floorf(x), -1.0e9f), 1.0e9f)); }

// Tap `i` along an axis of `n` texels under the boundary mode: its index in [0, n) in `r`; false when the tap reads 0
// (zero mode, out of range).
__device__ __forceinline__ bool resolve_tap(int i, int n, int boundary, int &r)
{
    if (boundary == kWrap) {
        r = i % n;
        if (r < 0) r += n;                 // a true modulo
        return true;
    }
    r = min(max(i, 0), n - 1);
    return boundary == kClamp || r == i;
}

__global__ __launch_bounds__(kBlock) void texture_nearest_kernel(const float *tex, int64_t tex_batch, int tex_h, int tex_w, int channels,
                                                                 const float2 *uv, int64_t pixels, int64_t per_image, int boundary, float *out)
{
    const int64_t gid = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (gid >= pixels) return;
    const float2 p = uv[gid];
    int rx, ry;
    const bool in_x = resolve_tap(floor_index(p.x * float(tex_w)), tex_w, boundary, rx);
    const bool in_y = resolve_tap(floor_index(p.y * float(tex_h)), tex_h, boundary, ry);
    const float *t = tex + (tex_batch > 1 ? gid / per_image : 0) * tex_h * tex_w * channels + (int64_t(ry) * tex_w + rx) * channels;
    float *o = out + gid * channels;
    for (int c = 0; c < channels; ++c) o[c] = in_x && in_y ? t[c] : 0.f;
}

__global__ __launch_bounds__(kBlock) void texture_nearest_backward_kernel(int64_t tex_batch, int tex_h, int tex_w, int channels, const float2 *uv,
                                                                          int64_t pixels, int64_t per_image, int boundary, const float *grad_out,
                                                                          float *grad_tex)
{
    const int64_t gid = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (gid >= pixels) return;
    const float2 p = uv[gid];
    int rx, ry;
    const bool in_x = resolve_tap(floor_index(p.x * float(tex_w)), tex_w, boundary, rx);
    const bool in_y = resolve_tap(floor_index(p.y * float(tex_h)), tex_h, boundary, ry);
    if (!in_x || !in_y) return;
    float *t = grad_tex + (tex_batch > 1 ? gid / per_image : 0) * tex_h * tex_w * channels + (int64_t(ry) * tex_w + rx) * channels;
    const float *g = grad_out + gid * channels;
    for (int c = 0; c < channels; ++c) atomicAdd(t + c, g[c]);
}

// The four taps of a bilinear lookup: x = u W - 0.5, y = v H - 0.5, taps at floor and floor + 1, weights from the fractions.
struct Taps {
    int64_t o00, o10, o01, o11;     // offsets (floats) of tap (x0, y0), (x1, y0), (x0, y1), (x1, y1) inside one texture
    bool in00, in10, in01, in11;    // false: the tap reads 0 and receives no gradient
    float fx, fy;
};

__device__ __forceinline__ Taps bilinear_taps(float2 p, int tex_h, int tex_w, int channels, int boundary)
{
    const float x = p.x * float(tex_w) - 0.5f, y = p.y * float(tex_h) - 0.5f;
    const int ix = floor_index(x), iy = floor_index(y);
    int x0, x1, y0, y1;
    const bool bx0 = resolve_tap(ix, tex_w, boundary, x0), bx1 = resolve_tap(ix + 1, tex_w, boundary, x1);
    const bool by0 = resolve_tap(iy, tex_h, boundary, y0), by1 = resolve_tap(iy + 1, tex_h, boundary, y1);
    Taps t;
    t.o00 = (int64_t(y0) * tex_w + x0) * channels, t.o10 = (int64_t(y0) * tex_w + x1) * channels;
    t.o01 = (int64_t(y1) * tex_w + x0) * channels, t.o11 = (int64_t(y1) * tex_w + x1) * channels;
    t.in00 = bx0 && by0, t.in10 = bx1 && by0, t.in01 = bx0 && by1, t.in11 = bx1 && by1;
    t.fx = x - floorf(x), t.fy = y - floorf(y);
    return t;
}

__global__ __launch_bounds__(kBlock) void texture_linear_kernel(const float *tex, int64_t tex_batch, int tex_h, int tex_w, int channels,
                                                                const float2 *uv, int64_t pixels, int64_t per_image, int boundary, float *out)
{
    const int64_t gid = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (gid >= pixels) return;
    const Taps t = bilinear_taps(uv[gid], tex_h, tex_w, channels, boundary);
    const float *tb = tex + (tex_batch > 1 ? gid / per_image : 0) * tex_h * tex_w * channels;
    const float w00 = (1.f - t.fx) * (1.f - t.fy), w10 = t.fx * (1.f - t.fy), w01 = (1.f - t.fx) * t.fy, w11 = t.fx * t.fy;
    float *o = out + gid * channels;
    for (int c = 0; c < channels; ++c) {
        const float t00 = t.in00 ? tb[t.o00 + c] : 0.f, t10 = t.in10 ? tb[t.o10 + c] : 0.f;
        const float t01 = t.in01 ? tb[t.o01 + c] : 0.f, t11 = t.in11 ? tb[t.o11 + c] : 0.f;
        o[c] = w00 * t00 + w10 * t10 + w01 * t01 + w11 * t11;
    }
}

// dL/dtex: w g into each tap of non-zero weight that exists; dL/du = W sum_c g_c ((t10 - t00)(1 - fy) + (t11 - t01) fy) and
// dL/dv = H sum_c g_c ((t01 - t00)(1 - fx) + (t11 - t10) fx), from the taps actually used (two clamped taps that coincide
// give 0).  tex may be null when grad_uv is.
__global__ __launch_bounds__(kBlock) void texture_linear_backward_kernel(const float *tex, int64_t tex_batch, int tex_h, int tex_w, int channels,
                                                                         const float2 *uv, int64_t pixels, int64_t per_image, int boundary,
                                                                         const float *grad_out, float *grad_tex, float2 *grad_uv)
{
    const int64_t gid = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (gid >= pixels) return;
    const Taps t = bilinear_taps(uv[gid], tex_h, tex_w, channels, boundary);
    const int64_t base = (tex_batch > 1 ? gid / per_image : 0) * tex_h * tex_w * channels;
    const float w00 = (1.f - t.fx) * (1.f - t.fy), w10 = t.fx * (1.f - t.fy), w01 = (1.f - t.fx) * t.fy, w11 = t.fx * t.fy;
    const float *g = grad_out + gid * channels;
    float du = 0.f, dv = 0.f;
    for (int c = 0; c < channels; ++c) {
        const float gc = g[c];
        if (grad_tex) {
            float *gt = grad_tex + base + c;
            if (t.in00 && w00 != 0.f) atomicAdd(gt + t.o00, w00 * gc);
            if (t.in10 && w10 != 0.f) atomicAdd(gt + t.o10, w10 * gc);
            if (t.in01 && w01 != 0.f) atomicAdd(gt + t.o01, w01 * gc);
            if (t.in11 && w11 != 0.f) atomicAdd(gt + t.o11, w11 * gc);
        }
        if (grad_uv) {
            const float *tb = tex + base + c;
            const float t00 = t.in00 ? tb[t.o00] : 0.f, t10 = t.in10 ? tb[t.o10] : 0.f;
            const float t01 = t.in01 ? tb[t.o01] : 0.f, t11 = t.in11 ? tb[t.o11] : 0.f;
            du += gc * ((t10 - t00) * (1.f - t.fy) + (t11 - t01) * t.fy);
            dv += gc * ((t01 - t00) * (1.f - t.fx) + (t11 - t10) * t.fx);
        }
    }
    if (grad_uv) grad_uv[gid] = make_float2(float(tex_w) * du, float(tex_h) * dv);
}

}  // namespace

hipError_t launch_atlas_bake_positions(const float *v_pos, int64_t n_vertices, const int32_t *tri, int64_t n_triangles, int32_t texture_res,
                                       const AtlasLayout &lay, float *positions, int32_t *owner, hipStream_t stream)
{
    const int64_t texels = int64_t(texture_res) * texture_res;
    if (texels <= 0) return hipSuccess;
    hipLaunchKernelGGL(atlas_bake_kernel, dim3(blocks_for(texels)), dim3(kBlock), 0, stream, v_pos, n_vertices, tri, n_triangles, texture_res, lay,
                       positions, owner);
    return hipGetLastError();
}

hipError_t launch_texture(const float *tex, int64_t tex_batch, int32_t tex_h, int32_t tex_w, int32_t channels, const float *uv, int64_t pixels,
                          int64_t pixels_per_image, int filter, int boundary, float *out, hipStream_t stream)
{
    if (pixels <= 0) return hipSuccess;
    const float2 *uv2 = reinterpret_cast<const float2 *>(uv);
    if (filter == 0)
        hipLaunchKernelGGL(texture_nearest_kernel, dim3(blocks_for(pixels)), dim3(kBlock), 0, stream, tex, tex_batch, tex_h, tex_w, channels, uv2,
                           pixels, pixels_per_image, boundary, out);
    else
        hipLaunchKernelGGL(texture_linear_kernel, dim3(blocks_for(pixels)), dim3(kBlock), 0, stream, tex, tex_batch, tex_h, tex_w, channels, uv2,
                           pixels, pixels_per_image, boundary, out);
    return hipGetLastError();
}

hipError_t launch_texture_backward(const float *tex, int64_t tex_batch, int32_t tex_h, int32_t tex_w, int32_t channels, const float *uv,
                                   int64_t pixels, int64_t pixels_per_image, int filter, int boundary, const float *grad_out, float *grad_tex,
                                   float *grad_uv, hipStream_t stream)
{
    if (grad_tex) {
        const hipError_t e = hipMemsetAsync(grad_tex, 0, size_t(tex_batch) * size_t(tex_h) * size_t(tex_w) * size_t(channels) * sizeof(float), stream);
        if (e != hipSuccess) return e;
    }
    if (pixels <= 0 || (!grad_tex && !grad_uv)) return hipSuccess;
    const float2 *uv2 = reinterpret_cast<const float2 *>(uv);
    if (filter == 0) {
        if (!grad_tex) return hipSuccess;
        hipLaunchKernelGGL(texture_nearest_backward_kernel, dim3(blocks_for(pixels)), dim3(kBlock), 0, stream, tex_batch, tex_h, tex_w, channels, uv2,
                           pixels, pixels_per_image, boundary, grad_out, grad_tex);
    } else {
        hipLaunchKernelGGL(texture_linear_backward_kernel, dim3(blocks_for(pixels)), dim3(kBlock), 0, stream, tex, tex_batch, tex_h, tex_w, channels,
                           uv2, pixels, pixels_per_image, boundary, grad_out, grad_tex, reinterpret_cast<float2 *>(grad_uv));
    }
    return hipGetLastError();
}

}  // namespace tsamd
