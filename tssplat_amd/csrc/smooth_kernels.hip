// gfx950 kernels of the surface smoother: vertex adjacency from sorted 64-bit keys, and the Taubin / tangential half-step.
//   smooth_keys_kernel       one lane per face: the validity byte (three indices in range, pairwise distinct), six directed edge keys
//                            src << 32 | dst (both directions of the three edges) and three vertex-face keys vertex << 32 | t; an
//                            invalid face writes the sentinel 2^63 - 1 nine times.  Nothing is read through an index
//   smooth_rows_kernel       one lane per position of the SORTED edge keys.  The first position of a run of equal keys is one
//                            neighbour (head = 1); it walks its run, whose length is the number of valid faces at that edge, and a
//                            length other than two marks the run's source vertex irregular: a plain store of 1, and the opposite
//                            run marks the other end, so there are no atomics.  The walk is bounded by the key count
//   smooth_classify_kernel   one lane per vertex: moves, or the first reason why not (other, pinned, irregular)
//   smooth_step_kernel       one half-step from a source state to a DIFFERENT destination state.  One lane per vertex walks its row
//                            of neighbours (and, tangential, its list of faces) serially: the sums live in the lane's registers, so
//                            their order is the row's order whatever the execution order.  A held vertex is copied, so either buffer
//                            is complete after any number of half-steps.  Every loop is bounded by a row length, and a row, neighbour
//                            or face entry that a correct adjacency cannot hold makes the vertex a copy instead of an access out of
//                            bounds.  A hub vertex is walked by ONE lane: its wave waits for it
// Semantics: tests/smooth_oracle.py.  Every operation is rounded on its own (-ffp-contract=off, _build.py; IEEE division), no float
// atomics: the results are bitwise repeatable and equal the oracle's.
// State layout: n_vertices records of `stride` float64, stride 3 (24 bytes: one record in eight straddles a 128-byte line) or 4
// (32 bytes, 32-byte aligned: never straddles, a third more bytes; read as one 16-byte and one 8-byte load).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "smooth.h"

namespace tsamd {

namespace {

constexpr int kBlock = kSmoothBlock;

__device__ inline bool finite_bits(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

inline unsigned blocks_for(int64_t n) { return unsigned((n + kBlock - 1) / kBlock); }

__global__ __launch_bounds__(kBlock) void smooth_keys_kernel(const int32_t *__restrict__ faces, int64_t n_triangles, int64_t n_vertices,
                                                             uint8_t *__restrict__ valid, int64_t *__restrict__ edge_keys, int64_t *__restrict__ face_keys)
{
    const int64_t t = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (t >= n_triangles) return;
    const int64_t a = faces[t * 3], b = faces[t * 3 + 1], c = faces[t * 3 + 2];
    const bool ok = a >= 0 && b >= 0 && c >= 0 && a < n_vertices && b < n_vertices && c < n_vertices && a != b && b != c && a != c;
    valid[t] = ok ? 1 : 0;
    int64_t *e = edge_keys + t * 6;
    e[0] = ok ? ((a << 32) | b) : kSmoothSentinel;
    e[1] = ok ? ((b << 32) | a) : kSmoothSentinel;
    e[2] = ok ? ((b << 32) | c) : kSmoothSentinel;
    e[3] = ok ? ((c << 32) | b) : kSmoothSentinel;
    e[4] = ok ? ((c << 32) | a) : kSmoothSentinel;
    e[5] = ok ? ((a << 32) | c) : kSmoothSentinel;
    int64_t *f = face_keys + t * 3;
    f[0] = ok ? ((a << 32) | t) : kSmoothSentinel;
    f[1] = ok ? ((b << 32) | t) : kSmoothSentinel;
    f[2] = ok ? ((c << 32) | t) : kSmoothSentinel;
}

__global__ __launch_bounds__(kBlock) void smooth_rows_kernel(const int64_t *__restrict__ keys, int64_t n_keys, int64_t n_vertices, uint8_t *__restrict__ head,
                                                             uint8_t *__restrict__ irregular)
{
    const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n_keys) return;
    const int64_t key = keys[i];
    const bool first = key != kSmoothSentinel && (i == 0 || keys[i - 1] != key);
    head[i] = first ? 1 : 0;
    if (!first) return;
    int64_t len = 1;
    for (int64_t j = i + 1; j < n_keys && keys[j] == key; ++j) ++len;        // bounded by the key count known at launch
    const int64_t src = key >> 32;
    if (len != 2 && src >= 0 && src < n_vertices) irregular[src] = 1;        // every writer stores the same 1
}

__global__ __launch_bounds__(kBlock) void smooth_classify_kernel(const float *__restrict__ v, SmoothMesh m, const uint8_t *__restrict__ irregular,
                                                                 const uint8_t *__restrict__ pinned, int32_t boundary_free, uint8_t *__restrict__ cls)
{
    const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= m.n_vertices) return;
    const int64_t r0 = m.offsets[i], r1 = m.offsets[i + 1];
    bool ok = finite_bits(v[i * 3]) && finite_bits(v[i * 3 + 1]) && finite_bits(v[i * 3 + 2]) && r0 >= 0 && r1 > r0 && r1 <= m.n_neighbours;
    if (ok) {
        for (int64_t k = r0; k < r1; ++k) {                                  // bounded by the row length
            const int64_t j = m.neighbours[k];
            if (j < 0 || j >= m.n_vertices) {
                ok = false;
                break;
            }
            ok = ok && finite_bits(v[j * 3]) && finite_bits(v[j * 3 + 1]) && finite_bits(v[j * 3 + 2]);
        }
    }
    uint8_t c = kSmoothMoves;
    if (!ok)
        c = kSmoothHeldOther;
    else if (pinned && pinned[i])
        c = kSmoothHeldPinned;
    else if (!boundary_free && irregular[i])
        c = kSmoothHeldIrregular;
    cls[i] = c;
}

template <int Stride>
__device__ inline void load_point(const double *__restrict__ state, int64_t i, double &x, double &y, double &z)
{
    if constexpr (Stride == 4) {
        const double2 xy = *reinterpret_cast<const double2 *>(state + i * 4);
        x = xy.x;
        y = xy.y;
        z = state[i * 4 + 2];
    } else {
        x = state[i * 3];
        y = state[i * 3 + 1];
        z = state[i * 3 + 2];
    }
}

template <int Stride>
__device__ inline void store_point(double *__restrict__ state, int64_t i, double x, double y, double z)
{
    if constexpr (Stride == 4) {
        *reinterpret_cast<double2 *>(state + i * 4) = make_double2(x, y);
        *reinterpret_cast<double2 *>(state + i * 4 + 2) = make_double2(z, 0.0);
    } else {
        state[i * 3] = x;
        state[i * 3 + 1] = y;
        state[i * 3 + 2] = z;
    }
}

__device__ inline double clamp_to(double q, double lo, double hi) { return q < lo ? lo : (q > hi ? hi : q); }   // a NaN passes through

template <int Stride, bool Tangential>
__global__ __launch_bounds__(kBlock) void smooth_step_kernel(const double *__restrict__ src, double *__restrict__ dst, SmoothMesh m,
                                                             const uint8_t *__restrict__ cls, double coef, const float *__restrict__ v0, double max_move)
{
    const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= m.n_vertices) return;
    double px, py, pz;
    load_point<Stride>(src, i, px, py, pz);
    double qx = px, qy = py, qz = pz;
    const int64_t r0 = m.offsets[i], r1 = m.offsets[i + 1];
    bool ok = cls[i] == kSmoothMoves && r0 >= 0 && r1 > r0 && r1 <= m.n_neighbours;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    if (ok) {
        for (int64_t k = r0; k < r1; ++k) {                                  // bounded by the row length
            const int64_t j = m.neighbours[k];
            if (j < 0 || j >= m.n_vertices) {
                ok = false;
                break;
            }
            double x, y, z;
            load_point<Stride>(src, j, x, y, z);
            sx += x;
            sy += y;
            sz += z;
        }
    }
    if (ok) {
        const double deg = double(r1 - r0);
        const double dx = coef * (sx / deg - px), dy = coef * (sy / deg - py), dz = coef * (sz / deg - pz);
        if constexpr (!Tangential) {
            qx = px + dx;
            qy = py + dy;
            qz = pz + dz;
        } else {
            const int64_t f0 = m.face_offsets[i], f1 = m.face_offsets[i + 1];
            ok = f0 >= 0 && f1 >= f0 && f1 <= m.n_face_entries;
            double nx = 0.0, ny = 0.0, nz = 0.0;
            for (int64_t k = f0; ok && k < f1; ++k) {                        // bounded by the list length
                const int64_t t = m.faces_of[k];
                if (t < 0 || t >= m.n_triangles) {
                    ok = false;
                    break;
                }
                const int64_t a = m.faces[t * 3], b = m.faces[t * 3 + 1], c = m.faces[t * 3 + 2];
                if (a < 0 || b < 0 || c < 0 || a >= m.n_vertices || b >= m.n_vertices || c >= m.n_vertices) {
                    ok = false;
                    break;
                }
                double ax, ay, az, bx, by, bz, cx, cy, cz;
                load_point<Stride>(src, a, ax, ay, az);
                load_point<Stride>(src, b, bx, by, bz);
                load_point<Stride>(src, c, cx, cy, cz);
                const double ux = bx - ax, uy = by - ay, uz = bz - az, wx = cx - ax, wy = cy - ay, wz = cz - az;
                nx += uy * wz - uz * wy;
                ny += uz * wx - ux * wz;
                nz += ux * wy - uy * wx;
            }
            const double nn = (nx * nx + ny * ny) + nz * nz;
            if (ok && nn > 0.0) {
                const double s = ((dx * nx + dy * ny) + dz * nz) / nn;
                qx = px + (dx - nx * s);
                qy = py + (dy - ny * s);
                qz = pz + (dz - nz * s);
            }
        }
        if (ok && v0) {
            const double cx = double(v0[i * 3]), cy = double(v0[i * 3 + 1]), cz = double(v0[i * 3 + 2]);
            qx = clamp_to(qx, cx - max_move, cx + max_move);
            qy = clamp_to(qy, cy - max_move, cy + max_move);
            qz = clamp_to(qz, cz - max_move, cz + max_move);
        }
        if (!ok) qx = px, qy = py, qz = pz;
    }
    store_point<Stride>(dst, i, qx, qy, qz);
}

}  // namespace

hipError_t launch_smooth_keys(const int32_t *faces, int64_t n_triangles, int64_t n_vertices, uint8_t *valid, int64_t *edge_keys, int64_t *face_keys,
                              hipStream_t stream)
{
    if (n_triangles == 0) return hipSuccess;
    hipLaunchKernelGGL(smooth_keys_kernel, dim3(blocks_for(n_triangles)), dim3(kBlock), 0, stream, faces, n_triangles, n_vertices, valid, edge_keys, face_keys);
    return hipGetLastError();
}

hipError_t launch_smooth_rows(const int64_t *sorted_keys, int64_t n_keys, int64_t n_vertices, uint8_t *head, uint8_t *irregular, hipStream_t stream)
{
    if (n_vertices > 0) {
        hipError_t e = hipMemsetAsync(irregular, 0, size_t(n_vertices), stream);
        if (e != hipSuccess) return e;
    }
    if (n_keys == 0) return hipSuccess;
    hipLaunchKernelGGL(smooth_rows_kernel, dim3(blocks_for(n_keys)), dim3(kBlock), 0, stream, sorted_keys, n_keys, n_vertices, head, irregular);
    return hipGetLastError();
}

hipError_t launch_smooth_classify(const float *v, const SmoothMesh &mesh, const uint8_t *irregular, const uint8_t *pinned, int32_t boundary_free,
                                  uint8_t *cls, hipStream_t stream)
{
    if (mesh.n_vertices == 0) return hipSuccess;
    hipLaunchKernelGGL(smooth_classify_kernel, dim3(blocks_for(mesh.n_vertices)), dim3(kBlock), 0, stream, v, mesh, irregular, pinned, boundary_free, cls);
    return hipGetLastError();
}

hipError_t launch_smooth_step(const double *src, double *dst, int32_t stride, const SmoothMesh &mesh, const uint8_t *cls, int32_t mode, double coef,
                              const float *v0, double max_move, hipStream_t stream)
{
    if (mesh.n_vertices == 0) return hipSuccess;
    const dim3 grid(blocks_for(mesh.n_vertices)), block(kBlock);
    if (stride == 4 && mode == kSmoothTangential)
        hipLaunchKernelGGL((smooth_step_kernel<4, true>), grid, block, 0, stream, src, dst, mesh, cls, coef, v0, max_move);
    else if (stride == 4)
        hipLaunchKernelGGL((smooth_step_kernel<4, false>), grid, block, 0, stream, src, dst, mesh, cls, coef, v0, max_move);
    else if (mode == kSmoothTangential)
        hipLaunchKernelGGL((smooth_step_kernel<3, true>), grid, block, 0, stream, src, dst, mesh, cls, coef, v0, max_move);
    else
        hipLaunchKernelGGL((smooth_step_kernel<3, false>), grid, block, 0, stream, src, dst, mesh, cls, coef, v0, max_move);
    return hipGetLastError();
}

}  // namespace tsamd
