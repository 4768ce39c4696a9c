// gfx950 kernels of the surface metrics: area-uniform surface samples and the all-pairs nearest-point search under them.
//   sample_weights_kernel    one lane per triangle: the float64 length w of (b - a) x (c - a), and its maximum through an integer
//                            atomicMax on the bits of w (w >= +0, so the bits order like the value)
//   sample_quantise_kernel   one lane per triangle, in place: q = floor((w / w_max) 2^32), 0 for a triangle that cannot be drawn
//   sample_draw_kernel       one lane per sample: three counter-based 64-bit draws, the triangle by an upper-bound binary search in
//                            the prefix sums of q, the point from two 24-bit barycentrics in float32, the float64 unit face normal
//   nearest_points_kernel    brute force.  A workgroup keeps kNearestBlock x kNearestQueriesPerLane queries in registers and streams
//                            its chunk of the ref points through LDS in tiles of kNearestTile, read at a wave-uniform address (one
//                            broadcast LDS read per ref point and wave).  Per pair: three differences, three products, two sums in
//                            exactly the order of the definition; per group of 8 ref points the unsigned minimum of the 8 bit
//                            patterns (v_min3_u32), and only where that improves on the query's best -- rare once the stream is a
//                            few thousand points old -- a scan of the group for the lowest index that holds it.  The partial
//                            minimum of a chunk goes into the query's 64-bit key (bits(d2) << 32 | index) by atomicMin
//   nearest_finish_kernel    key -> (d2, index); an untouched key gives (+inf, -1)
// Semantics: tests/metrics_oracle.py.  Every operation is rounded on its own (-ffp-contract=off, _build.py; IEEE division and
// square root); d2 is a sum of squares, so it is never negative and never -0: as unsigned integers its bits order like its value,
// +inf (0x7F800000) included, and every NaN lies above (a NaN that comes out of an operation is quiet: >= 0x7FC00000).  The minimum is taken on integers: no float atomics, the results are
// bitwise repeatable, independent of the chunk count, and equal the oracle's.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mesh_triangle.h"
#include "metrics.h"

namespace tsamd {

namespace {

constexpr int kBlock = 256;

// splitmix64's finaliser over seed + (counter + 1) golden-ratio increments: draw `counter` of the stream `seed`
__device__ inline uint64_t mix64(uint64_t seed, uint64_t counter)
{
    uint64_t z = seed + (counter + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ __launch_bounds__(kBlock) void sample_weights_kernel(const float *__restrict__ v, int64_t n_vertices, const int32_t *__restrict__ faces,
                                                                int64_t n_triangles, int64_t *__restrict__ weights, unsigned long long *wmax)
{
    const int64_t t = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (t >= n_triangles) return;
    Triangle tri;
    double w = 0.0;
    if (load_triangle(v, n_vertices, faces, t, tri)) {
        double nx, ny, nz;
        w = face_normal(tri, nx, ny, nz);
    }
    unsigned long long bits = (unsigned long long)__double_as_longlong(w);
    if (!(w > 0.0) || (bits & 0x7FF0000000000000ull) == 0x7FF0000000000000ull) bits = 0;      // zero area, or not finite: never drawn
    weights[t] = (int64_t)bits;
    // the maximum only grows, so a stale read can only cause an atomic that changes nothing
    if (bits > __atomic_load_n(wmax, __ATOMIC_RELAXED)) atomicMax(wmax, bits);
}

__global__ __launch_bounds__(kBlock) void sample_quantise_kernel(int64_t n_triangles, int64_t *__restrict__ weights, const unsigned long long *__restrict__ wmax)
{
    const int64_t t = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (t >= n_triangles) return;
    const double w = __longlong_as_double(weights[t]), top = __longlong_as_double((long long)*wmax);
    weights[t] = w > 0.0 ? (int64_t)(unsigned long long)floor((w / top) * 4294967296.0) : 0;   // <= 2^32
}

__global__ __launch_bounds__(kBlock) void sample_draw_kernel(const float *__restrict__ v, int64_t n_vertices, const int32_t *__restrict__ faces,
                                                             int64_t n_triangles, const int64_t *__restrict__ prefix, int64_t n_samples, uint64_t seed,
                                                             float *__restrict__ points, float *__restrict__ normals, int32_t *__restrict__ tri_out)
{
    const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n_samples) return;
    const uint64_t total = (uint64_t)prefix[n_triangles - 1];
    const uint64_t p = __umul64hi(mix64(seed, 3 * uint64_t(i)), total);                        // uniform in [0, total)
    int64_t lo = 0, hi = n_triangles;                                                          // the first t with prefix[t] > p
    while (lo < hi) {                                                                          // at most 32 halvings
        const int64_t mid = (lo + hi) >> 1;
        if ((uint64_t)prefix[mid] > p) hi = mid; else lo = mid + 1;
    }
    const int64_t t = lo < n_triangles ? lo : n_triangles - 1;                                 // (only a prefix that is no prefix sum gets here)
    uint32_t ia = uint32_t(mix64(seed, 3 * uint64_t(i) + 1) >> 40), ib = uint32_t(mix64(seed, 3 * uint64_t(i) + 2) >> 40);
    if (ia + ib > (1u << 24)) {                                                                // a + b > 1, decided exactly
        ia = (1u << 24) - ia;
        ib = (1u << 24) - ib;
    }
    const float a = float(ia) * 0x1p-24f, b = float(ib) * 0x1p-24f;                            // both exact
    const float nan = __uint_as_float(0x7FC00000u);
    float px = nan, py = nan, pz = nan, mx = nan, my = nan, mz = nan;
    Triangle tri;
    if (load_triangle(v, n_vertices, faces, t, tri)) {                                         // always, under a prefix made from these faces
        px = (tri.a[0] + a * (tri.b[0] - tri.a[0])) + b * (tri.c[0] - tri.a[0]);
        py = (tri.a[1] + a * (tri.b[1] - tri.a[1])) + b * (tri.c[1] - tri.a[1]);
        pz = (tri.a[2] + a * (tri.b[2] - tri.a[2])) + b * (tri.c[2] - tri.a[2]);
        double nx, ny, nz;
        const double w = face_normal(tri, nx, ny, nz);
        mx = float(nx / w);
        my = float(ny / w);
        mz = float(nz / w);
    }
    points[i * 3] = px;
    points[i * 3 + 1] = py;
    points[i * 3 + 2] = pz;
    normals[i * 3] = mx;
    normals[i * 3 + 1] = my;
    normals[i * 3 + 2] = mz;
    tri_out[i] = int32_t(t);
}

constexpr int kQ = kNearestQueriesPerLane;
constexpr int kTile = kNearestTile;
constexpr uint32_t kNoPair = 0x7F800001u;          // just above the bits of +inf: +inf replaces it, a NaN (above it) does not

__global__ __launch_bounds__(kNearestBlock) void nearest_points_kernel(const float *__restrict__ query, int64_t n, const float *__restrict__ ref, int64_t m,
                                                                       int64_t per_chunk, unsigned long long *keys)
{
    __shared__ float4 tile[kTile];
    const int64_t q0 = int64_t(blockIdx.x) * (kNearestBlock * kQ) + threadIdx.x;
    float qx[kQ], qy[kQ], qz[kQ];
    uint32_t best[kQ];
    int32_t arg[kQ];
#pragma unroll
    for (int k = 0; k < kQ; ++k) {
        int64_t q = q0 + int64_t(k) * kNearestBlock;
        if (q > n - 1) q = n - 1;                              // a lane past the end repeats the last query and stores nothing
        qx[k] = query[q * 3];
        qy[k] = query[q * 3 + 1];
        qz[k] = query[q * 3 + 2];
        best[k] = kNoPair;
        arg[k] = -1;
    }
    const int64_t first = int64_t(blockIdx.y) * per_chunk;     // workgroup-uniform, like the loop bounds below
    const int64_t last = first + per_chunk < m ? first + per_chunk : m;
    const float nan = __uint_as_float(0x7FC00000u);
    for (int64_t base = first; base < last; base += kTile) {
        const int32_t count = int32_t(last - base < kTile ? last - base : kTile);
        const int32_t padded = (count + 7) & ~7;               // <= kTile; the padding is NaN, which never wins
        __syncthreads();                                       // the previous tile has been read by every wave
        for (int32_t j = threadIdx.x; j < padded; j += kNearestBlock) {
            float4 p = make_float4(nan, nan, nan, 0.0f);
            if (j < count) {
                const float *r = ref + (base + j) * 3;
                p = make_float4(r[0], r[1], r[2], 0.0f);
            }
            tile[j] = p;
        }
        __syncthreads();
        for (int32_t j = 0; j < padded; j += 8) {
float4 r[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) r[u] = tile[j + u];
#pragma unroll
            for (int k = 0; k < kQ; ++k) {
                uint32_t bits[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const float dx = qx[k] - r[u].x, dy = qy[k] - r[u].y, dz = qz[k] - r[u].z;
                    bits[u] = __float_as_uint((dx * dx + dy * dy) + dz * dz);
                }
                const uint32_t m = min(min(min(bits[0], bits[1]), min(bits[2], bits[3])), min(min(bits[4], bits[5]), min(bits[6], bits[7])));
                if (m < best[k]) {                             // rare once the stream is a few thousand points old
                    best[k] = m;
                    int32_t at = 7;
#pragma unroll
                    for (int u = 6; u >= 0; --u) at = bits[u] == m ? u : at;
                    arg[k] = int32_t(base) + j + at;           // the lowest index of the group's minimum
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kQ; ++k) {
        const int64_t q = q0 + int64_t(k) * kNearestBlock;
        if (q < n && arg[k] >= 0) atomicMin(keys + q, ((unsigned long long)best[k] << 32) | (unsigned long long)uint32_t(arg[k]));
    }
}

__global__ __launch_bounds__(kBlock) void nearest_finish_kernel(const unsigned long long *__restrict__ keys, int64_t n, float *__restrict__ d2_out,
                                                                int32_t *__restrict__ idx_out)
{
    const int64_t q = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (q >= n) return;
    const unsigned long long key = keys[q];
    const bool none = key == ~0ull;                            // no pair without a NaN
    d2_out[q] = __uint_as_float(none ? 0x7F800000u : uint32_t(key >> 32));
    idx_out[q] = none ? -1 : int32_t(uint32_t(key));
}

inline unsigned blocks_for(int64_t items) { return unsigned((items + kBlock - 1) / kBlock); }

}  // namespace

hipError_t launch_sample_weights(const float *v, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, int64_t *weights, uint64_t *wmax,
                                 hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(wmax, 0, sizeof(uint64_t), stream);
    if (e != hipSuccess) return e;
    auto *top = reinterpret_cast<unsigned long long *>(wmax);
    hipLaunchKernelGGL(sample_weights_kernel, dim3(blocks_for(n_triangles)), dim3(kBlock), 0, stream, v, n_vertices, faces, n_triangles, weights, top);
    hipLaunchKernelGGL(sample_quantise_kernel, dim3(blocks_for(n_triangles)), dim3(kBlock), 0, stream, n_triangles, weights, top);
    return hipGetLastError();
}

hipError_t launch_sample_draw(const float *v, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, const int64_t *prefix, int64_t n_samples,
                              uint64_t seed, float *points_out, float *normals_out, int32_t *tri_out, hipStream_t stream)
{
    hipLaunchKernelGGL(sample_draw_kernel, dim3(blocks_for(n_samples)), dim3(kBlock), 0, stream, v, n_vertices, faces, n_triangles, prefix, n_samples, seed,
                       points_out, normals_out, tri_out);
    return hipGetLastError();
}

hipError_t launch_nearest_points(const float *query, int64_t n, const float *ref, int64_t m, int32_t chunks, uint64_t *keys, float *d2_out,
                                 int32_t *idx_out, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(keys, 0xFF, size_t(n) * sizeof(uint64_t), stream);
    if (e != hipSuccess) return e;
    auto *k = reinterpret_cast<unsigned long long *>(keys);
    const int64_t per_chunk = (m + chunks - 1) / chunks;
    const int64_t per_block = int64_t(kNearestBlock) * kQ;
    hipLaunchKernelGGL(nearest_points_kernel, dim3(unsigned((n + per_block - 1) / per_block), unsigned(chunks)), dim3(kNearestBlock), 0, stream, query, n, ref, m,
                       per_chunk, k);
    hipLaunchKernelGGL(nearest_finish_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, stream, k, n, d2_out, idx_out);
    return hipGetLastError();
}

}  // namespace tsamd
