// Device helpers shared by the kernels that read a triangle of an indexed mesh (metrics_kernels.hip, pointmesh_kernels.hip): the
// guarded load and the float64 face normal whose length is the sampler's weight w (tests/metrics_oracle.py: face_normals).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace tsamd {

__device__ inline bool finite_bits(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

struct Triangle {
    float a[3], b[3], c[3];
};

// false when an index is outside [0, n_vertices) or a coordinate is not finite; nothing is read through a bad index
__device__ inline bool load_triangle(const float *__restrict__ v, int64_t n_vertices, const int32_t *__restrict__ faces, int64_t t, Triangle &tri)
{
    const int32_t ia = faces[t * 3], ib = faces[t * 3 + 1], ic = faces[t * 3 + 2];
    if (ia < 0 || ib < 0 || ic < 0 || ia >= n_vertices || ib >= n_vertices || ic >= n_vertices) return false;
    bool ok = true;
    for (int x = 0; x < 3; ++x) {
        tri.a[x] = v[int64_t(ia) * 3 + x];
        tri.b[x] = v[int64_t(ib) * 3 + x];
        tri.c[x] = v[int64_t(ic) * 3 + x];
        ok = ok && finite_bits(tri.a[x]) && finite_bits(tri.b[x]) && finite_bits(tri.c[x]);
    }
    return ok;
}

// (b - a) x (c - a) in float64, each component two rounded products and a difference, and its length (merge_kernels.hip: face_plane)
__device__ inline double face_normal(const Triangle &tri, double &nx, double &ny, double &nz)
{
    const double ux = double(tri.b[0]) - double(tri.a[0]), uy = double(tri.b[1]) - double(tri.a[1]), uz = double(tri.b[2]) - double(tri.a[2]);
    const double wx = double(tri.c[0]) - double(tri.a[0]), wy = double(tri.c[1]) - double(tri.a[1]), wz = double(tri.c[2]) - double(tri.a[2]);
    nx = uy * wz - uz * wy;
    ny = uz * wx - ux * wz;
    nz = ux * wy - uy * wx;
    return __dsqrt_rn((nx * nx + ny * ny) + nz * nz);
}

}  // namespace tsamd
