// gfx950 kernels of the exact point-to-triangle search (tsamd_nearest_on_mesh): for every query the closest triangle of a mesh.
//   pointmesh_prepare_kernel  one lane per triangle: validity (the guarded load and the sampler's w > 0), the three corners, and a
//                             float32 bounding sphere -- the centroid rounded to float32 and a radius rounded UP, see the margin below;
//                             the centre once more as a packed ref point of the seeding search (NaN for an invalid triangle)
//   pointmesh_seed_kernel     one lane per query: the triangle whose sphere centre is nearest (tsamd_nearest_points over the centres)
//                             is evaluated exactly and becomes the query's first key, so that the bound bites from the first tile
//   pointmesh_search_kernel   shaped like nearest_points_kernel: kPointMeshBlock x kPointMeshQueriesPerLane queries in registers, the
//                             chunk's spheres streamed through LDS in tiles and read at wave-uniform addresses.  Per pair a float32
//                             test "can this sphere hold a point as close as the best so far"; per group of 8 spheres, only where
//                             one passes, the float64 evaluation of those that pass.  The partial result goes into the query's key
//                             bits(fl32 d2) << 32 | triangle by a 64-bit atomicMin
//   pointmesh_finish_kernel   key -> (d2, triangle) and the closest point, recomputed from the winning triangle by the same operations
// Semantics: tests/pointmesh_oracle.py -- Ericson's Voronoi regions in float64 on the float32 inputs, every operation rounded on its own
// (-ffp-contract=off, _build.py; IEEE division and square root), in the operation order of include/tssplat_amd.h.  d2 is a sum of squares:
// never negative, never -0, so the bits of fl32(d2) order like its value and the minimum is taken on integers; the key's low word makes
// the lowest triangle win a tie.  The sphere test and the seed decide which pairs are evaluated, never what an evaluated pair gives: the
// result is the minimum over ALL valid triangles, bitwise repeatable and independent of the chunk count.
//
// The margin.  A pair is evaluated unless, in float32, dc2 > (r' + s')^2 with dc2 = ((qx - cx)^2 + (qy - cy)^2) + (qz - cz)^2 the squared
// distance to the stored centre c, r' the stored radius and s' the query's slack.  No pair with fl32(d2) <= B (B the query's best so
// far, equality included) may be skipped.  Write u = 2^-24, rho for the exact radius of the corners about the STORED centre, S for
// the largest |coordinate| of c, d for the exact distance from the query to the triangle and D^2 for the float64 value the
// evaluation returns.
//   (1) The kernel stores r' >= rho + 2^-18 (S + rho) + 2^-60: rho is computed in float64 about the float32 centre (relative error
//       below 2^-50), widened by 2^-17 (S + rho) + 2^-60 and rounded to float32 upwards.  s' = fl(sqrt(B)) (1 + 2^-17) >= sqrt(B) (1 + 2^-18).
//   (2) float32 rounding: dc2 is five roundings above exact data (the differences of stored float32 values are single roundings), the
//       right side three; r' >= 2^-60 keeps the square a normal number, and an underflow on the left only lowers it.  So a skipped pair
//       has dc > (r' + s') (1 - 5u) in exact arithmetic, hence d >= dc - rho > sqrt(B) (1 + 2^-19) + 2^-19 (S + rho).  Overflow to +inf on the
//       left needs a real value above FLT_MAX; on the right it keeps the pair.  A NaN on the left (a NaN query) is a pair whose d2 is NaN.
//   (3) The float64 evaluation.  In a vertex or an edge region the barycentrics are 0, 1 or a quotient a / (a + b) of two numbers of one
//       sign, so X lies on the triangle whatever the roundings were, up to the 2^-52 |X| of its own three operations: D >= d - 2^-50 (S + rho + d).
//       Only the interior branch can put X off the triangle, and then within its plane, by (excess of v, w or 1 - v - w) x L, L the longest
//       edge; h is the height over it, so s = (va + vb) + vc = (L h)^2 up to rounding.  Each d_i is L times the tangential offset of the
//       query, at most L l with l the distance from the projection of the query to the triangle plus L, and carries an absolute error of
//       2^-52 L R, R = d + 2 rho the largest |AP|, |BP|, |CP|; a product d_i d_j so carries 2^-50 L^2 R l.
//       (a) l <= 4 L, the projection on or near the triangle -- the only place where a true barycentric is near 0: the barycentrics are
//           off by at most 2^-48 R L / h^2, X by L times that, and with h >= 2^-8 L (a thinner triangle gets r' = +inf and is never
//           skipped) D >= d - 2^-32 R, whatever R is.
//       (b) l > 4 L: the exact closest point lies on the boundary and the exact va, vb or vc that says so has the size L^2 h l against
//           an error of 2^-50 L^2 R l: the sign is right, and a vertex or edge region is taken, while R < 2^48 h.  Beyond that -- a query
//           more than 2^40 of its radii away from a triangle, with the float32 lattice aimed along a normal whose products do not come
//           out exact -- this argument ends; between the two scales of such a pair lie more bits than a float32 coordinate holds.
//       In both cases D >= d - 2^-30 (S + rho + d).
//   Together D > sqrt(B) (1 + 2^-20), D^2 > B (1 + 2^-20), and as rounding to float32 is monotone and the next float32 above B is at most
//   B (1 + 2^-23), fl32(D^2) > B (for B = 0: D > 2^-61, whose square is a normal float32).  An invalid triangle stores NaN and fails every
//   comparison; with no best yet, or a best of +inf, s' = +inf and everything is evaluated.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mesh_triangle.h"
#include "metrics.h"
#include "pointmesh.h"

namespace tsamd {

namespace {

constexpr int kBlock = kPointMeshBlock;             // the one-lane-per-item kernels use the search's workgroup size
constexpr int kQ = kPointMeshQueriesPerLane;
constexpr int kTile = kPointMeshTile;
constexpr unsigned long long kNoKey = ~0ull;        // no pair yet: above every key of a real pair

// Ericson, Real-Time Collision Detection 5.1.5, in the operation order of tests/pointmesh_oracle.py; X = (A + AB v) + AC w.
// Every region's barycentrics are one quotient each (x / 1 is exact), so the seven regions cost two divisions, not a branch each.
__device__ inline double closest_point(float qx, float qy, float qz, const float4 A, const float4 B, const float4 C, double &xx, double &xy, double &xz)
{
    const double px = qx, py = qy, pz = qz, ax = A.x, ay = A.y, az = A.z;
    const double abx = double(B.x) - ax, aby = double(B.y) - ay, abz = double(B.z) - az;
    const double acx = double(C.x) - ax, acy = double(C.y) - ay, acz = double(C.z) - az;
    const double apx = px - ax, apy = py - ay, apz = pz - az;
    const double bpx = px - double(B.x), bpy = py - double(B.y), bpz = pz - double(B.z);
    const double cpx = px - double(C.x), cpy = py - double(C.y), cpz = pz - double(C.z);
    const double d1 = (abx * apx + aby * apy) + abz * apz, d2 = (acx * apx + acy * apy) + acz * apz;
    const double d3 = (abx * bpx + aby * bpy) + abz * bpz, d4 = (acx * bpx + acy * bpy) + acz * bpz;
    const double d5 = (abx * cpx + aby * cpy) + abz * cpz, d6 = (acx * cpx + acy * cpy) + acz * cpz;
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const double e = d4 - d3, g = d5 - d6;
    double vn, vd = 1.0, wn, wd = 1.0;
    bool bc = false;
    if (d1 <= 0.0 && d2 <= 0.0) {                           // vertex A
        vn = 0.0, wn = 0.0;
    } else if (d3 >= 0.0 && d4 <= d3) {                     // vertex B
        vn = 1.0, wn = 0.0;
    } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {       // edge AB
        vn = d1, vd = d1 - d3, wn = 0.0;
    } else if (d6 >= 0.0 && d5 <= d6) {                     // vertex C
        vn = 0.0, wn = 1.0;
    } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {       // edge AC
        vn = 0.0, wn = d2, wd = d2 - d6;
    } else if (va <= 0.0 && e >= 0.0 && g >= 0.0) {         // edge BC: v = 1 - w
        vn = 0.0, wn = e, wd = e + g, bc = true;
    } else {                                                // interior
        const double s = (va + vb) + vc;
        vn = vb, vd = s, wn = vc, wd = s;
    }
    const double w = wn / wd;
    const double v = bc ? 1.0 - w : vn / vd;
    xx = (ax + abx * v) + acx * w;
    xy = (ay + aby * v) + acy * w;
    xz = (az + abz * v) + acz * w;
    const double dx = px - xx, dy = py - xy, dz = pz - xz;
    return (dx * dx + dy * dy) + dz * dz;
}

// bits(fl32 d2) << 32 | t, or kNoKey for a NaN
__device__ inline unsigned long long pair_key(double d2, int32_t t)
{
    if (!(d2 == d2)) return kNoKey;
    return ((unsigned long long)__float_as_uint(float(d2)) << 32) | (unsigned long long)uint32_t(t);
}

// s' of the margin: +inf while there is no best or the best is +inf
__device__ inline float slack(unsigned long long key)
{
    const uint32_t bits = uint32_t(key >> 32);
    if (bits >= 0x7F800000u) return __uint_as_float(0x7F800000u);
    return sqrtf(__uint_as_float(bits)) * (1.0f + 0x1p-17f);
}

__device__ inline bool sphere_may_hold(float qx, float qy, float qz, const float4 s, float slack)
{
    const float dx = qx - s.x, dy = qy - s.y, dz = qz - s.z, reach = s.w + slack;
    return (dx * dx + dy * dy) + dz * dz <= reach * reach;          // false for a NaN: an invalid triangle, tile padding, a NaN query
}

__global__ __launch_bounds__(kBlock) void pointmesh_prepare_kernel(const float *__restrict__ v, int64_t n_vertices, const int32_t *__restrict__ faces,
                                                                   int64_t n_triangles, float4 *__restrict__ spheres, float4 *__restrict__ corners,
                                                                   float *__restrict__ centres)
{
    const int64_t t = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (t >= n_triangles) return;
    const float nan = __uint_as_float(0x7FC00000u);
    float4 sphere = make_float4(nan, nan, nan, nan), a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a, c = a;
    Triangle tri;
    if (load_triangle(v, n_vertices, faces, t, tri)) {
        double nx, ny, nz;
        const double w = face_normal(tri, nx, ny, nz);
        if (w > 0.0) {
            float cf[3];
            double rr = 0.0, edge = 0.0, top = 0.0;
            for (int x = 0; x < 3; ++x) cf[x] = float(((double(tri.a[x]) + double(tri.b[x])) + double(tri.c[x])) / 3.0);
            double ra = 0.0, rb = 0.0, rc = 0.0, ab = 0.0, ac = 0.0, bc = 0.0;
            for (int x = 0; x < 3; ++x) {
                const double pa = double(tri.a[x]), pb = double(tri.b[x]), pc = double(tri.c[x]), m = double(cf[x]);
                ra += (pa - m) * (pa - m);
                rb += (pb - m) * (pb - m);
                rc += (pc - m) * (pc - m);
                ab += (pb - pa) * (pb - pa);
                ac += (pc - pa) * (pc - pa);
                bc += (pc - pb) * (pc - pb);
                top = fmax(top, fabs(m));
            }
            rr = __dsqrt_rn(fmax(ra, fmax(rb, rc)));
            edge = fmax(ab, fmax(ac, bc));                           // L^2; w = L h
            rr = rr + 0x1p-17 * (top + rr) + 0x1p-60;
            float r = float(rr);
            if (double(r) < rr) r = __uint_as_float(__float_as_uint(r) + 1u);      // upwards: r > 0, so the next bit pattern (+inf after FLT_MAX)
            if (!(w >= 0x1p-8 * edge)) r = __uint_as_float(0x7F800000u);           // h < 2^-8 L: never skipped
            sphere = make_float4(cf[0], cf[1], cf[2], r);
            a = make_float4(tri.a[0], tri.a[1], tri.a[2], 0.0f);
            b = make_float4(tri.b[0], tri.b[1], tri.b[2], 0.0f);
            c = make_float4(tri.c[0], tri.c[1], tri.c[2], 0.0f);
        }
    }
    spheres[t] = sphere;
    corners[t * 3] = a;
    corners[t * 3 + 1] = b;
    corners[t * 3 + 2] = c;
    centres[t * 3] = sphere.x;
    centres[t * 3 + 1] = sphere.y;
    centres[t * 3 + 2] = sphere.z;
}

__global__ __launch_bounds__(kBlock) void pointmesh_seed_kernel(const float *__restrict__ query, int64_t n, const float4 *__restrict__ corners,
                                                                int64_t n_triangles, const int32_t *__restrict__ seed_idx, unsigned long long *__restrict__ keys)
{
    const int64_t q = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (q >= n) return;
    const int32_t t = seed_idx[q];                                  // a valid triangle (an invalid one's centre is NaN), or -1
    unsigned long long key = kNoKey;
    if (t >= 0 && t < n_triangles) {
        double xx, xy, xz;
        key = pair_key(closest_point(query[q * 3], query[q * 3 + 1], query[q * 3 + 2], corners[int64_t(t) * 3], corners[int64_t(t) * 3 + 1],
                                     corners[int64_t(t) * 3 + 2], xx, xy, xz), t);
    }
    keys[q] = key;
}

__global__ __launch_bounds__(kPointMeshBlock) void pointmesh_search_kernel(const float *__restrict__ query, int64_t n, const float4 *__restrict__ spheres,
                                                                           const float4 *__restrict__ corners, int64_t n_triangles, int64_t per_chunk,
                                                                           unsigned long long *keys)
{
    __shared__ float4 tile[kTile];
    const int64_t q0 = int64_t(blockIdx.x) * (kPointMeshBlock * kQ) + threadIdx.x;
    float qx[kQ], qy[kQ], qz[kQ], reach[kQ];
    unsigned long long best[kQ];
#pragma unroll
    for (int k = 0; k < kQ; ++k) {
        int64_t q = q0 + int64_t(k) * kPointMeshBlock;
        if (q > n - 1) q = n - 1;                              // a lane past the end repeats the last query and stores nothing
        qx[k] = query[q * 3];
        qy[k] = query[q * 3 + 1];
        qz[k] = query[q * 3 + 2];
        // the seed, or what other chunks have made of it since: any key is the exact value of some valid triangle, so a stale or
        // a fresh read changes the work done, never the minimum
        best[k] = __atomic_load_n(keys + q, __ATOMIC_RELAXED);
        reach[k] = slack(best[k]);
    }
    const int64_t first = int64_t(blockIdx.y) * per_chunk;     // workgroup-uniform, like the loop bounds below
    const int64_t last = first + per_chunk < n_triangles ? first + per_chunk : n_triangles;
    const float nan = __uint_as_float(0x7FC00000u);
    for (int64_t base = first; base < last; base += kTile) {
        const int32_t count = int32_t(last - base < kTile ? last - base : kTile);
        const int32_t padded = (count + 7) & ~7;               // <= kTile; the padding is NaN, which fails the sphere test
        __syncthreads();                                       // the previous tile has been read by every wave
        for (int32_t j = threadIdx.x; j < padded; j += kPointMeshBlock) tile[j] = j < count ? spheres[base + j] : make_float4(nan, nan, nan, nan);
        __syncthreads();
        for (int32_t j = 0; j < padded; j += 8) {
            float4 s[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) s[u] = tile[j + u];
#pragma unroll
            for (int k = 0; k < kQ; ++k) {
                bool any = false;
#pragma unroll
                for (int u = 0; u < 8; ++u) any |= sphere_may_hold(qx[k], qy[k], qz[k], s[u], reach[k]);
                if (any) {
#pragma unroll 1
                    for (int u = 0; u < 8; ++u) {
                        if (!sphere_may_hold(qx[k], qy[k], qz[k], tile[j + u], reach[k])) continue;      // with the slack as it is by now
                        const int64_t t = base + j + u;        // < last: the padding never gets here
                        double xx, xy, xz;
                        const unsigned long long key = pair_key(closest_point(qx[k], qy[k], qz[k], corners[t * 3], corners[t * 3 + 1], corners[t * 3 + 2], xx, xy, xz),
                                                                int32_t(t));
                        if (key < best[k]) {
                            best[k] = key;
                            reach[k] = slack(key);
                        }
                    }
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kQ; ++k) {
        const int64_t q = q0 + int64_t(k) * kPointMeshBlock;
        if (q < n && best[k] != kNoKey) atomicMin(keys + q, best[k]);
    }
}

__global__ __launch_bounds__(kBlock) void pointmesh_finish_kernel(const float *__restrict__ query, int64_t n, const float4 *__restrict__ corners,
                                                                  int64_t n_triangles, const unsigned long long *__restrict__ keys, float *__restrict__ d2_out,
                                                                  int32_t *__restrict__ tri_out, float *__restrict__ point_out)
{
    const int64_t q = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (q >= n) return;
    const unsigned long long key = keys[q];
    const int64_t t = key == kNoKey ? -1 : int64_t(uint32_t(key));
    const bool none = t < 0 || t >= n_triangles;               // no pair without a NaN (a key is only ever written from a triangle below n_triangles)
    d2_out[q] = __uint_as_float(none ? 0x7F800000u : uint32_t(key >> 32));
    tri_out[q] = none ? -1 : int32_t(t);
    if (!point_out) return;
    const float nan = __uint_as_float(0x7FC00000u);
    float x = nan, y = nan, z = nan;
    if (!none) {
        double xx, xy, xz;
        closest_point(query[q * 3], query[q * 3 + 1], query[q * 3 + 2], corners[t * 3], corners[t * 3 + 1], corners[t * 3 + 2], xx, xy, xz);
        x = float(xx), y = float(xy), z = float(xz);
    }
    point_out[q * 3] = x;
    point_out[q * 3 + 1] = y;
    point_out[q * 3 + 2] = z;
}

inline unsigned blocks_for(int64_t items) { return unsigned((items + kBlock - 1) / kBlock); }

}  // namespace

hipError_t launch_nearest_on_mesh(const float *query, int64_t n, const float *v, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, int32_t chunks,
                                  void *workspace, float *d2_out, int32_t *tri_out, float *point_out, hipStream_t stream)
{
    const PointMeshWorkspace w = pointmesh_workspace(n, n_triangles);
    char *base = static_cast<char *>(workspace);
    auto *keys = reinterpret_cast<unsigned long long *>(base + w.keys);
    auto *spheres = reinterpret_cast<float4 *>(base + w.spheres);
    auto *corners = reinterpret_cast<float4 *>(base + w.corners);
    auto *centres = reinterpret_cast<float *>(base + w.centres);
    auto *seed_idx = reinterpret_cast<int32_t *>(base + w.seed_idx);
    hipLaunchKernelGGL(pointmesh_prepare_kernel, dim3(blocks_for(n_triangles)), dim3(kBlock), 0, stream, v, n_vertices, faces, n_triangles, spheres, corners,
                       centres);
    hipError_t e = launch_nearest_points(query, n, centres, n_triangles, nearest_auto_chunks(n, n_triangles), reinterpret_cast<uint64_t *>(base + w.seed_keys),
                                         reinterpret_cast<float *>(base + w.seed_d2), seed_idx, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pointmesh_seed_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, stream, query, n, corners, n_triangles, seed_idx, keys);
    const int64_t per_chunk = (n_triangles + chunks - 1) / chunks;
    const int64_t per_block = int64_t(kPointMeshBlock) * kQ;
    hipLaunchKernelGGL(pointmesh_search_kernel, dim3(unsigned((n + per_block - 1) / per_block), unsigned(chunks)), dim3(kPointMeshBlock), 0, stream, query, n, spheres,
                       corners, n_triangles, per_chunk, keys);
    hipLaunchKernelGGL(pointmesh_finish_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, stream, query, n, corners, n_triangles, keys, d2_out, tri_out, point_out);
    return hipGetLastError();
}

}  // namespace tsamd
