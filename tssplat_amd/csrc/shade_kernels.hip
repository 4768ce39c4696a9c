// gfx950 kernels of the texture stage's image side under a blend plan (include/tssplat_amd.h, tsamd_shade*): composite of the
// [N, 3] point colours over the background, antialias as the plan's fixed sparse operator, and the L1 loss against a target
// with its backward -- without a [B, H, W, .] temporary in either direction, without atomics, bitwise repeatable.
//
// The operation order is part of the contract (tests/shade_oracle.py derives its rounding bound from it), float32 throughout,
// every difference, product and sum rounded on its own (-ffp-contract=off, tssplat_amd/_build.py: SOURCE_FLAGS):
//   forward    out = c_p;  for the records r of destination p, in the order of the plan:  out = out + w_r * (c_src(r) - c_p)
//   backward   a = w_0;  a = a + w_r (records of destination p, in order);  acc = g_p * (1 - a)      [acc = g_p without records]
//              for the records r of source p, in order:  acc = acc + w_r * g_dst(r)
//   loss       d = out - t in float32, |d| and every sum in float64: lanes stride over the pixels, a fixed tree per workgroup, the
//              partials added in a fixed order by a second kernel, float(sum / n)
#include <hip/hip_runtime.h>

#include "det_mean.h"
#include "shade.h"

namespace tsamd {
namespace {

constexpr int kBlock = kMeanBlock;   // (the loss kernel sums its lanes with det_mean.h's tree)
constexpr int kMaxBlocks = 2048;     // 8 workgroups per CU: the loss kernel's fixed grid, one pixel per lane and pass

struct Rgb {
    float x, y, z;
};

__device__ __forceinline__ Rgb load3(const float *p, int64_t row) { return Rgb{p[3 * row], p[3 * row + 1], p[3 * row + 2]}; }
__device__ __forceinline__ void store3(float *p, int64_t row, Rgb v) { p[3 * row] = v.x, p[3 * row + 1] = v.y, p[3 * row + 2] = v.z; }

// the colour of pixel `pix` before antialiasing; `point` is its pix_point entry (anything outside [0, n_points) is background)
__device__ __forceinline__ Rgb pixel_colour(const tsamd_blend_plan &P, const float *color, const float *background, int64_t pix, int32_t point)
{
    return (point >= 0 && int64_t(point) < P.n_points) ? load3(color, point) : load3(background, pix);
}

// record range of slot `slot` of a CSR with `n_slots` rows, clipped to the n_blends records there are
__device__ __forceinline__ void record_range(const int32_t *ptr, int64_t n_slots, int64_t n_blends, int32_t slot, int64_t &r0, int64_t &r1)
{
    r0 = r1 = 0;
    if (slot < 0 || int64_t(slot) >= n_slots) return;
    const int64_t a = ptr[slot], b = ptr[slot + 1];
    r0 = a < 0 ? 0 : a;
    r1 = b > n_blends ? n_blends : b;
}

// out_p (see the head of the file)
// (`point`, `slot`: the pixel's pix_point and pix_dst entries, read once by the caller)
__device__ __forceinline__ Rgb shade_pixel(const tsamd_blend_plan &P, const float *color, const float *background, int64_t pixels, int64_t pix, int32_t point, int32_t slot)
{
    const Rgb c = pixel_colour(P, color, background, pix, point);
    Rgb out = c;
    int64_t r0, r1;
    record_range(P.dst_ptr_dev, P.n_dst, P.n_blends, slot, r0, r1);
    for (int64_t r = r0; r < r1; ++r) {
        const int32_t sp = P.dst_src_pix_dev[r];
        if (sp < 0 || int64_t(sp) >= pixels) continue;
        const Rgb s = pixel_colour(P, color, background, sp, P.dst_src_point_dev[r]);
        const float w = P.dst_weight_dev[r];
        out.x = out.x + w * (s.x - c.x);
        out.y = out.y + w * (s.y - c.y);
        out.z = out.z + w * (s.z - c.z);
    }
    return out;
}

__device__ __forceinline__ float sign_of(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }   // sign(0) = 0, sign(NaN) = 0

__global__ __launch_bounds__(kBlock) void shade_kernel(tsamd_blend_plan P, const float *color, const float *background, int64_t pixels, float *out)
{
    const int64_t pix = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (pix >= pixels) return;
    store3(out, pix, shade_pixel(P, color, background, pixels, pix, P.pix_point_dev[pix], P.pix_dst_dev[pix]));
}

// grad_color of point k from g(pixel, destination slot): the gradient of the loss at a pixel that is a point's own or a destination
template <class G>
__device__ __forceinline__ Rgb point_gradient(const tsamd_blend_plan &P, int64_t pixels, int64_t k, Rgb own, G &&g)
{
    int64_t r0, r1;
    record_range(P.dst_ptr_dev, P.n_dst, P.n_blends, P.point_dst_dev[k], r0, r1);
    Rgb acc = own;
    if (r1 > r0) {
        float a = P.dst_weight_dev[r0];
        for (int64_t r = r0 + 1; r < r1; ++r) a = a + P.dst_weight_dev[r];
        const float keep = 1.f - a;
        acc.x = own.x * keep, acc.y = own.y * keep, acc.z = own.z * keep;
    }
    record_range(P.src_ptr_dev, P.n_src, P.n_blends, P.point_src_dev[k], r0, r1);
    for (int64_t r = r0; r < r1; ++r) {
        const int32_t dp = P.src_dst_pix_dev[r], ds = P.src_dst_slot_dev[r];
        if (dp < 0 || int64_t(dp) >= pixels || ds < 0 || int64_t(ds) >= P.n_dst) continue;
        const Rgb gd = g(dp, ds);
        const float w = P.src_weight_dev[r];
        acc.x = acc.x + w * gd.x;
        acc.y = acc.y + w * gd.y;
        acc.z = acc.z + w * gd.z;
    }
    return acc;
}

__global__ __launch_bounds__(kBlock) void shade_backward_kernel(tsamd_blend_plan P, const float *grad_out, int64_t pixels, float *grad_color)
{
    const int64_t k = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (k >= P.n_points) return;
    const int32_t pix = P.point_pix_dev[k];
    Rgb acc{0.f, 0.f, 0.f};
    if (pix >= 0 && int64_t(pix) < pixels)
        acc = point_gradient(P, pixels, k, load3(grad_out, pix), [&](int32_t dp, int32_t) { return load3(grad_out, dp); });
    store3(grad_color, k, acc);
}

__global__ __launch_bounds__(kBlock) void shade_l1_backward_kernel(tsamd_blend_plan P, const float *point_sign, const float *dst_sign, const float *grad_loss, int64_t pixels,
                                                                   float *grad_color)
{
    const int64_t k = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (k >= P.n_points) return;
    const float scale = *grad_loss / float(3 * pixels);
    const Rgb s = load3(point_sign, k);
    const Rgb acc = point_gradient(P, pixels, k, Rgb{s.x * scale, s.y * scale, s.z * scale}, [&](int32_t, int32_t ds) {
        const Rgb d = load3(dst_sign, ds);
        return Rgb{d.x * scale, d.y * scale, d.z * scale};
    });
    store3(grad_color, k, acc);
}

__global__ __launch_bounds__(kBlock) void shade_l1_kernel(tsamd_blend_plan P, const float *color, const float *background, const float *target, int target_channels,
                                                          int64_t pixels, double *partials, float *image_out, float *point_sign, float *dst_sign)
{
    __shared__ double lds[kBlock / 64];
    const int64_t stride = int64_t(gridDim.x) * kBlock;
    double acc = 0.0;
    for (int64_t pix = int64_t(blockIdx.x) * kBlock + threadIdx.x; pix < pixels; pix += stride) {
        const int32_t k = P.pix_point_dev[pix], slot = P.pix_dst_dev[pix];
        const Rgb out = shade_pixel(P, color, background, pixels, pix, k, slot);
        const float *t = target + pix * target_channels;
        const float d0 = out.x - t[0], d1 = out.y - t[1], d2 = out.z - t[2];
        acc += (fabs(double(d0)) + fabs(double(d1))) + fabs(double(d2));
        if (image_out) store3(image_out, pix, out);
        if (point_sign) {
            const Rgb s{sign_of(d0), sign_of(d1), sign_of(d2)};
            if (k >= 0 && int64_t(k) < P.n_points) store3(point_sign, k, s);
            if (slot >= 0 && int64_t(slot) < P.n_dst) store3(dst_sign, slot, s);
        }
    }
    const double sum = block_sum(acc, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}

unsigned blocks_for(int64_t n) { return unsigned((n + kBlock - 1) / kBlock); }
int l1_blocks(int64_t pixels) { return mean_blocks(pixels, kBlock, kMaxBlocks); }
int64_t pixels_of(const tsamd_blend_plan &plan) { return plan.batch * int64_t(plan.height) * plan.width; }

}  // namespace

hipError_t launch_shade(const tsamd_blend_plan &plan, const float *color, const float *background, float *out, hipStream_t stream)
{
    const int64_t pixels = pixels_of(plan);
    if (pixels <= 0) return hipSuccess;
    hipLaunchKernelGGL(shade_kernel, dim3(blocks_for(pixels)), dim3(kBlock), 0, stream, plan, color, background, pixels, out);
    return hipGetLastError();
}

hipError_t launch_shade_backward(const tsamd_blend_plan &plan, const float *grad_out, float *grad_color, hipStream_t stream)
{
    if (plan.n_points <= 0) return hipSuccess;
    hipLaunchKernelGGL(shade_backward_kernel, dim3(blocks_for(plan.n_points)), dim3(kBlock), 0, stream, plan, grad_out, pixels_of(plan), grad_color);
    return hipGetLastError();
}

int64_t shade_l1_workspace_bytes(int64_t pixels) { return mean_workspace_bytes(l1_blocks(pixels)); }

hipError_t launch_shade_l1(const tsamd_blend_plan &plan, const float *color, const float *background, const float *target, int target_channels, void *workspace,
                           float *loss, float *image_out, float *point_sign_out, float *dst_sign_out, hipStream_t stream)
{
    const int64_t pixels = pixels_of(plan);
    if (pixels <= 0) return hipMemsetAsync(loss, 0, sizeof(float), stream);
    const int blocks = l1_blocks(pixels);
    hipLaunchKernelGGL(shade_l1_kernel, dim3(blocks), dim3(kBlock), 0, stream, plan, color, background, target, target_channels, pixels, static_cast<double *>(workspace),
                       image_out, point_sign_out, dst_sign_out);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : launch_mean_final(workspace, blocks, 3 * pixels, loss, stream);
}

hipError_t launch_shade_l1_backward(const tsamd_blend_plan &plan, const float *point_sign, const float *dst_sign, const float *grad_loss, float *grad_color,
                                    hipStream_t stream)
{
    if (plan.n_points <= 0) return hipSuccess;
    hipLaunchKernelGGL(shade_l1_backward_kernel, dim3(blocks_for(plan.n_points)), dim3(kBlock), 0, stream, plan, point_sign, dst_sign, grad_loss, pixels_of(plan), grad_color);
    return hipGetLastError();
}

}  // namespace tsamd
