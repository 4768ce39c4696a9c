// gfx950 kernels of the renderer slice: interpolate, forward and backward -- the nvdiffrast operator that turns a `rast` image
// (raster_kernels.hip) and a vertex attribute into an image.  One lane per pixel; 16 B of rast pixel in, `channels` floats out, the
// vertex gathers cached.  The triangle decode and the run scan are raster_device.h's.
#include <hip/hip_runtime.h>

#include "raster.h"
#include "raster_device.h"

namespace tsamd {
namespace {

// (these two kernels never need a row or a column, only the view, and only at a covered pixel: gid / hw, not locate_pixel)
__global__ __launch_bounds__(256) void interpolate_kernel(const float *attr, int64_t attr_batch, int64_t n_vertices, int channels,
                                                          const float4 *rast, const int32_t *tri, int64_t n_tri, int64_t batch, int64_t hw, float *out)
{
    const int64_t gid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (gid >= batch * hw) return;
    const float4 r = rast[gid];
    float *o = out + gid * channels;
    const int64_t t = triangle_of(r.w, n_tri);
    int32_t i0 = 0, i1 = 0, i2 = 0;
    // a pixel whose id names no triangle of THIS list, or a triangle with a vertex index outside the attribute array, is
    // background (what nvdiffrast does with them): the rast image may come from another triangle list, or from the caller
    if (t < 0 || !triangle_indices(tri, t, n_vertices, i0, i1, i2)) {
        for (int c = 0; c < channels; ++c) o[c] = 0.f;
        return;
    }
    const int64_t b = gid / hw;
    const float *a = attr + (attr_batch > 1 ? b : 0) * n_vertices * channels;
    const float *a0 = a + int64_t(i0) * channels, *a1 = a + int64_t(i1) * channels, *a2 = a + int64_t(i2) * channels;
    const float u = r.x, v = r.y, w = 1.f - r.x - r.y;
    for (int c = 0; c < channels; ++c) o[c] = u * a0[c] + v * a1[c] + w * a2[c];
}

// d out / d attr: scatter of the three barycentric weights, summed over runs of equal triangles inside the wave first (fp32
// global atomics: the order of the additions, and so the last bits of the result, vary from run to run -- like nvdiffrast's
// own backward); d out / d (u, v) per pixel.
__global__ __launch_bounds__(256) void interpolate_backward_kernel(const float *attr, int64_t attr_batch, int64_t n_vertices, int channels,
                                                                   const float4 *rast, const int32_t *tri, int64_t n_tri, int64_t batch, int64_t hw,
                                                                   const float *grad_out, float *grad_attr, float4 *grad_rast)
{
    const int64_t gid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const bool inside = gid < batch * hw;
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (inside) r = rast[gid];
    const int64_t t = triangle_of(r.w, n_tri);
    int32_t i0 = 0, i1 = 0, i2 = 0;
    const bool valid = inside && t >= 0 && triangle_indices(tri, t, n_vertices, i0, i1, i2);   // (else background: no reads, no atomics)
    if (inside && !valid && grad_rast) grad_rast[gid] = make_float4(0.f, 0.f, 0.f, 0.f);
    const int64_t b = valid ? gid / hw : 0;
    const int64_t base = (attr_batch > 1 ? b : 0) * n_vertices * channels;
    int64_t o0 = 0, o1 = 0, o2 = 0;
    if (valid) o0 = base + int64_t(i0) * channels, o1 = base + int64_t(i1) * channels, o2 = base + int64_t(i2) * channels;
    const float u = r.x, v = r.y, w = 1.f - r.x - r.y;
    // lanes of one triangle (and attribute batch) in a row: one set of atomics per run
    const Runs runs = find_runs(valid ? (attr_batch > 1 ? b : 0) * (int64_t(1) << 32) + t : -1 - int64_t(threadIdx.x));
    float du = 0.f, dv = 0.f;
    for (int c = 0; c < channels; ++c) {
        const float gc = valid ? grad_out[gid * channels + c] : 0.f;
        const float s0 = run_sum(runs, u * gc), s1 = run_sum(runs, v * gc), s2 = run_sum(runs, w * gc);
        if (valid) {
            if (runs.last) {
                atomicAdd(grad_attr + o0 + c, s0);
                atomicAdd(grad_attr + o1 + c, s1);
                atomicAdd(grad_attr + o2 + c, s2);
            }
            const float a2 = attr[o2 + c];
            du += gc * (attr[o0 + c] - a2);
            dv += gc * (attr[o1 + c] - a2);
        }
    }
    if (valid && grad_rast) grad_rast[gid] = make_float4(du, dv, 0.f, 0.f);
}

}  // namespace

hipError_t launch_interpolate(const float *attr, int64_t attr_batch, int64_t n_vertices, int channels, const float *rast, const int32_t *tri,
                              int64_t n_tri, int64_t batch, int height, int width, float *out, hipStream_t stream)
{
    const int64_t hw = int64_t(height) * width;
    if (batch * hw <= 0) return hipSuccess;
    hipLaunchKernelGGL(interpolate_kernel, dim3(unsigned((batch * hw + 255) / 256)), dim3(256), 0, stream, attr, attr_batch, n_vertices, channels,
                       reinterpret_cast<const float4 *>(rast), tri, n_tri, batch, hw, out);
    return hipGetLastError();
}

hipError_t launch_interpolate_backward(const float *attr, int64_t attr_batch, int64_t n_vertices, int channels, const float *rast, const int32_t *tri,
                                       int64_t n_tri, int64_t batch, int height, int width, const float *grad_out, float *grad_attr, float *grad_rast,
                                       hipStream_t stream)
{
    const int64_t hw = int64_t(height) * width;
    hipError_t e = hipMemsetAsync(grad_attr, 0, size_t(attr_batch) * size_t(n_vertices) * size_t(channels) * sizeof(float), stream);
    if (e != hipSuccess) return e;
    if (batch * hw <= 0) return hipSuccess;
    hipLaunchKernelGGL(interpolate_backward_kernel, dim3(unsigned((batch * hw + 255) / 256)), dim3(256), 0, stream, attr, attr_batch, n_vertices, channels,
                       reinterpret_cast<const float4 *>(rast), tri, n_tri, batch, hw, grad_out, grad_attr, reinterpret_cast<float4 *>(grad_rast));
    return hipGetLastError();
}

}  // namespace tsamd
