// gfx950 kernels of the surface simplifier: vertex clustering on a cube grid with quadric placement.
//   simplify_vertex_keys_kernel   one lane per vertex: the cell key (i C + j) C + k, -1 for a coordinate that is not finite
//   simplify_records_kernel       one lane per triangle: its state (survives, degenerate, invalid) and three record slots
//                                 (cell << 32) | t, one per distinct cell among the corners' cells, the unused ones a sentinel that
//                                 sorts last.  Nothing is read through a bad index
//   simplify_run_walk_kernel      one lane per sorted record.  The lane of a run's first record (its predecessor holds another cell)
//                                 walks the run serially: 12 float64 sums and a count, one rounded add per term in ascending record
//                                 order, then the 3x3 solve by cofactors, the clamp and the position.  It also tells every slot of the
//                                 run, through the sort's permutation, where the run starts.  The walk is bounded by the slot count
//   simplify_faces_kernel         one lane per triangle: a survivor's three runs, rotated so that the smallest comes first (runs are
//                                 in ascending cell order, so that is the smallest cell key), and the two sort keys of the triple
//   simplify_dedupe_kernel        one lane per position of the sorted triples: equal to its predecessor -> a duplicate; every other
//                                 survivor is kept and marks its three runs as used (plain stores of 1)
// Semantics: tests/simplify_oracle.py.  Every operation is rounded on its own (-ffp-contract=off, _build.py; IEEE division).  No
// float atomics and no waiting on another workgroup: a cell's sums live in one lane's registers, so their order is the record
// order whatever the execution order, and the results are bitwise repeatable and equal the oracle's.  A record, permutation or
// order entry that cannot have come from the stage before raises the status word instead of an access out of bounds.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "simplify.h"

namespace tsamd {

namespace {

constexpr int kBlock = 256;

__device__ inline bool finite_bits(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }
__device__ inline bool finite_bits64(double v) { return ((unsigned long long)__double_as_longlong(v) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull; }

inline unsigned blocks_for(int64_t n) { return unsigned((n + kBlock - 1) / kBlock); }

__global__ __launch_bounds__(kBlock) void simplify_vertex_keys_kernel(const float *__restrict__ v, int64_t n_vertices, int32_t cells, double lo, double h,
                                                                      int32_t *__restrict__ vkey)
{
    const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n_vertices) return;
    const double top = double(cells - 1);
    int32_t key = 0;
    bool ok = true;
    for (int x = 0; x < 3; ++x) {
        const float p = v[i * 3 + x];
        ok = ok && finite_bits(p);
        double q = floor((double(p) - lo) / h);                          // p finite, h > 0: a number or an infinity, never a NaN
        if (q > top) q = top;
        if (q < 0.0) q = 0.0;
        key = key * cells + (ok ? int32_t(q) : 0);
    }
    vkey[i] = ok ? key : -1;
}

__global__ __launch_bounds__(kBlock) void simplify_records_kernel(const int32_t *__restrict__ faces, int64_t n_triangles, int64_t n_vertices,
                                                                  const int32_t *__restrict__ vkey, int64_t *__restrict__ records, uint8_t *__restrict__ state)
{
    const int64_t t = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (t >= n_triangles) return;
    const int32_t ia = faces[t * 3], ib = faces[t * 3 + 1], ic = faces[t * 3 + 2];
    int64_t r0 = kSimplifySentinel, r1 = kSimplifySentinel, r2 = kSimplifySentinel;
    uint8_t s = 2;
    if (ia >= 0 && ib >= 0 && ic >= 0 && ia < n_vertices && ib < n_vertices && ic < n_vertices) {
        const int32_t ka = vkey[ia], kb = vkey[ib], kc = vkey[ic];
        if (ka >= 0 && kb >= 0 && kc >= 0) {
            r0 = (int64_t(ka) << 32) | t;
            if (kb != ka) r1 = (int64_t(kb) << 32) | t;
            if (kc != ka && kc != kb) r2 = (int64_t(kc) << 32) | t;
            s = (ka != kb && ka != kc && kb != kc) ? 0 : 1;
        }
    }
    records[t * 3] = r0;
    records[t * 3 + 1] = r1;
    records[t * 3 + 2] = r2;
    state[t] = s;
}

__global__ __launch_bounds__(kBlock) void simplify_run_walk_kernel(const float *__restrict__ v, int64_t n_vertices, const int32_t *__restrict__ faces,
                                                                   int64_t n_triangles, int32_t cells, double lo, double h, int32_t placement, double stabilise,
                                                                   const int32_t *__restrict__ vkey, const int64_t *__restrict__ records,
                                                                   const int64_t *__restrict__ perm, int64_t n_slots, float *__restrict__ pos,
                                                                   uint8_t *__restrict__ head, int32_t *__restrict__ run, int32_t *status)
{
    const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n_slots) return;
    const int64_t key = records[i];
    if (key == kSimplifySentinel) return;
    const int64_t cell = key >> 32;
    if (i > 0 && (records[i - 1] >> 32) == cell) return;                 // not the first record of its run
    if (cell < 0 || cell >= int64_t(cells) * cells * cells) {
        atomicMax(status, kSimplifyStatusRecords);
        return;
    }
    const int32_t ci = int32_t(cell / (int64_t(cells) * cells)), cj = int32_t((cell / cells) % cells), ck = int32_t(cell % cells);
    const double g[3] = {lo + (double(ci) + 0.5) * h, lo + (double(cj) + 0.5) * h, lo + (double(ck) + 0.5) * h};
    double A00 = 0.0, A01 = 0.0, A02 = 0.0, A11 = 0.0, A12 = 0.0, A22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0, P0 = 0.0, P1 = 0.0, P2 = 0.0;
    int64_t count = 0, prev = -1;
    for (int64_t j = i; j < n_slots; ++j) {                              // bounded by the slot count known at launch
        const int64_t kj = records[j];
        if ((kj >> 32) != cell) break;                                   // the sentinel's upper half is no cell
        const int64_t t = kj & 0xFFFFFFFFll, slot = perm[j];
        if (kj <= prev || t >= n_triangles || slot < 0 || slot >= n_slots) {
            atomicMax(status, kSimplifyStatusRecords);
            break;
        }
        prev = kj;
        const int32_t ia = faces[t * 3], ib = faces[t * 3 + 1], ic = faces[t * 3 + 2];
        if (ia < 0 || ib < 0 || ic < 0 || ia >= n_vertices || ib >= n_vertices || ic >= n_vertices) {
            atomicMax(status, kSimplifyStatusRecords);
            break;
        }
        const int32_t ka = vkey[ia], kb = vkey[ib], kc = vkey[ic];
        if (ka < 0 || kb < 0 || kc < 0 || (ka != cell && kb != cell && kc != cell)) {
            atomicMax(status, kSimplifyStatusRecords);
            break;
        }
        run[slot] = int32_t(i);
        double a[3], e[3], f[3];
        for (int x = 0; x < 3; ++x) {
            a[x] = double(v[int64_t(ia) * 3 + x]);
            e[x] = double(v[int64_t(ib) * 3 + x]);
            f[x] = double(v[int64_t(ic) * 3 + x]);
        }
        const double ux = e[0] - a[0], uy = e[1] - a[1], uz = e[2] - a[2], wx = f[0] - a[0], wy = f[1] - a[1], wz = f[2] - a[2];
        const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
        const double ax = a[0] - g[0], ay = a[1] - g[1], az = a[2] - g[2];
        const double d = -((nx * ax + ny * ay) + nz * az);
        A00 += nx * nx;
        A01 += nx * ny;
        A02 += nx * nz;
        A11 += ny * ny;
        A12 += ny * nz;
        A22 += nz * nz;
        b0 += d * nx;
        b1 += d * ny;
        b2 += d * nz;
        if (ka == cell) {
            P0 += ax;
            P1 += ay;
            P2 += az;
            ++count;
        }
        if (kb == cell) {
            P0 += e[0] - g[0];
            P1 += e[1] - g[1];
            P2 += e[2] - g[2];
            ++count;
        }
        if (kc == cell) {
            P0 += f[0] - g[0];
            P1 += f[1] - g[1];
            P2 += f[2] - g[2];
            ++count;
        }
    }
    const double n = double(count);
    const double m[3] = {P0 / n, P1 / n, P2 / n};
    double x[3] = {m[0], m[1], m[2]};
    if (placement == kSimplifyQuadric) {
        const double tr = (A00 + A11) + A22;
        const double lam = stabilise * tr;
        const double M00 = A00 + lam, M01 = A01, M02 = A02, M11 = A11 + lam, M12 = A12, M22 = A22 + lam;
        const double r0 = lam * m[0] - b0, r1 = lam * m[1] - b1, r2 = lam * m[2] - b2;
        const double c00 = M11 * M22 - M12 * M12, c01 = M02 * M12 - M01 * M22, c02 = M01 * M12 - M02 * M11;
        const double c11 = M00 * M22 - M02 * M02, c12 = M01 * M02 - M00 * M12, c22 = M00 * M11 - M01 * M01;
        const double det = (M00 * c00 + M01 * c01) + M02 * c02;
        const double q0 = ((c00 * r0 + c01 * r1) + c02 * r2) / det;
        const double q1 = ((c01 * r0 + c11 * r1) + c12 * r2) / det;
        const double q2 = ((c02 * r0 + c12 * r1) + c22 * r2) / det;
        if (tr > 0.0 && det > 0.0 && finite_bits64(q0) && finite_bits64(q1) && finite_bits64(q2)) {
            x[0] = q0;
            x[1] = q1;
            x[2] = q2;
        }
    }
    const double half = 0.5 * h;
    uint8_t flags = 1;
    for (int c = 0; c < 3; ++c) {
        if (x[c] > half) {
            x[c] = half;
            flags = 3;
        } else if (x[c] < -half) {
            x[c] = -half;
            flags = 3;
        }
        pos[i * 3 + c] = float(g[c] + x[c]);
    }
    head[i] = flags;
}

__global__ __launch_bounds__(kBlock) void simplify_faces_kernel(const int32_t *__restrict__ run, const uint8_t *__restrict__ state, int64_t n_triangles,
                                                                int32_t *__restrict__ tri, int64_t *__restrict__ key_ab, int64_t *__restrict__ key_c)
{
    const int64_t t = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (t >= n_triangles) return;
    int32_t a = -1, b = -1, c = -1;
    if (state[t] == 0) {                                                 // three distinct cells: slot s is corner s
        const int32_t r0 = run[t * 3], r1 = run[t * 3 + 1], r2 = run[t * 3 + 2];
        if (r0 >= 0 && r1 >= 0 && r2 >= 0) {
            if (r0 < r1 && r0 < r2) {
                a = r0, b = r1, c = r2;
            } else if (r1 < r2) {
                a = r1, b = r2, c = r0;
            } else {
                a = r2, b = r0, c = r1;
            }
        }
    }
    tri[t * 3] = a;
    tri[t * 3 + 1] = b;
    tri[t * 3 + 2] = c;
    key_ab[t] = a < 0 ? kSimplifySentinel : ((int64_t(a) << 32) | int64_t(b));
    key_c[t] = a < 0 ? kSimplifySentinel : int64_t(c);
}

__global__ __launch_bounds__(kBlock) void simplify_dedupe_kernel(const int32_t *__restrict__ tri, const int64_t *__restrict__ order, int64_t n_triangles,
                                                                 uint8_t *__restrict__ keep, uint8_t *__restrict__ used, int32_t *status)
{
    const int64_t p = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (p >= n_triangles) return;
    const int64_t t = order[p];
    if (t < 0 || t >= n_triangles) {
        atomicMax(status, kSimplifyStatusOrder);
        return;
    }
    const int32_t a = tri[t * 3], b = tri[t * 3 + 1], c = tri[t * 3 + 2];
    if (a < 0) return;                                                   // no survivor: keep[t] stays 0
    if (p > 0) {
        const int64_t q = order[p - 1];
        if (q < 0 || q >= n_triangles) return;                           // (the lane of p - 1 raises the status word)
        if (tri[q * 3] == a && tri[q * 3 + 1] == b && tri[q * 3 + 2] == c) return;      // the same triple at a lower index
    }
    const int64_t n_slots = 3 * n_triangles;
    if (b < 0 || c < 0 || a >= n_slots || b >= n_slots || c >= n_slots) {
        atomicMax(status, kSimplifyStatusOrder);
        return;
    }
    keep[t] = 1;
    used[a] = 1;                                                         // every writer stores the same 1
    used[b] = 1;
    used[c] = 1;
}

}  // namespace

hipError_t launch_simplify_keys(const float *v, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, int32_t cells, double lo, double hi,
                                int32_t *vkey_out, int64_t *records_out, uint8_t *state_out, hipStream_t stream)
{
    const double h = (hi - lo) / double(cells);
    if (n_vertices > 0)
        hipLaunchKernelGGL(simplify_vertex_keys_kernel, dim3(blocks_for(n_vertices)), dim3(kBlock), 0, stream, v, n_vertices, cells, lo, h, vkey_out);
    if (n_triangles > 0)
        hipLaunchKernelGGL(simplify_records_kernel, dim3(blocks_for(n_triangles)), dim3(kBlock), 0, stream, faces, n_triangles, n_vertices, vkey_out, records_out,
                           state_out);
    return hipGetLastError();
}

hipError_t launch_simplify_cells(const float *v, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, int32_t cells, double lo, double hi,
                                 int32_t placement, double stabilise, const int32_t *vkey, const int64_t *records, const int64_t *perm, float *pos_out,
                                 uint8_t *head_out, int32_t *run_out, int32_t *status_out, hipStream_t stream)
{
    const int64_t n_slots = 3 * n_triangles;
    hipError_t e = hipMemsetAsync(status_out, 0, sizeof(int32_t), stream);
    if (e != hipSuccess) return e;
    if (n_slots == 0) return hipSuccess;
    if ((e = hipMemsetAsync(head_out, 0, size_t(n_slots), stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(run_out, 0xFF, size_t(n_slots) * sizeof(int32_t), stream)) != hipSuccess) return e;
    const double h = (hi - lo) / double(cells);
    hipLaunchKernelGGL(simplify_run_walk_kernel, dim3(blocks_for(n_slots)), dim3(kBlock), 0, stream, v, n_vertices, faces, n_triangles, cells, lo, h, placement,
                       stabilise, vkey, records, perm, n_slots, pos_out, head_out, run_out, status_out);
    return hipGetLastError();
}

hipError_t launch_simplify_faces(const int32_t *run, const uint8_t *state, int64_t n_triangles, int32_t *tri_out, int64_t *key_ab_out, int64_t *key_c_out,
                                 hipStream_t stream)
{
    if (n_triangles == 0) return hipSuccess;
    hipLaunchKernelGGL(simplify_faces_kernel, dim3(blocks_for(n_triangles)), dim3(kBlock), 0, stream, run, state, n_triangles, tri_out, key_ab_out, key_c_out);
    return hipGetLastError();
}

hipError_t launch_simplify_dedupe(const int32_t *tri, const int64_t *order, int64_t n_triangles, uint8_t *keep_out, uint8_t *used_out, int32_t *status_out,
                                  hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(status_out, 0, sizeof(int32_t), stream);
    if (e != hipSuccess) return e;
    if (n_triangles == 0) return hipSuccess;
    if ((e = hipMemsetAsync(keep_out, 0, size_t(n_triangles), stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(used_out, 0, size_t(3 * n_triangles), stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(simplify_dedupe_kernel, dim3(blocks_for(n_triangles)), dim3(kBlock), 0, stream, tri, order, n_triangles, keep_out, used_out, status_out);
    return hipGetLastError();
}

}  // namespace tsamd
