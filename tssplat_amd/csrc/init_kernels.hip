// gfx950 kernels of the sphere initialisation: silhouettes -> visual hull -> exact squared distance transform -> greedy ball cover.
//   occupancy_pack_kernel   alpha[..., c] > threshold as one bit per pixel, one ballot (64 pixels, two words) per wave
//   hull_carve_kernel       one lane per voxel, uniform loop over the views (matrices by scalar loads), a wave leaves it once a
//                           ballot shows none of its voxels still inside
//   edt_pass_kernel         out[a] = min_j f[j] + (a - j)^2 along one axis, lines staged in LDS; three launches, int32 throughout
//   greedy_cover_kernel     launch t clears the ball recorded by launch t - 1 and finds the next maximum of d2 over what is left:
//                           64-bit key (q << 32) | (0xFFFFFFFF - flat), wave shuffle, LDS, one integer atomicMax per workgroup
// Semantics: tests/spheres_init_oracle.py.  Everything a decision depends on is an integer, a separately rounded float32 operation
// (-ffp-contract=off, _build.py; IEEE division) or one double multiply and compare of exactly representable integers: the
// results are bitwise repeatable and equal the oracle's.  No float atomics, no square root.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "init.h"

namespace tsamd {

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kEdtLines = 16;        // lines per workgroup of an EDT pass: 16 x 512 x 4 B = 32 KiB of LDS at the largest grid
constexpr int kCoverBlocks = 2048;   // grid-stride: eight workgroups per CU

// rows = batch x height image rows; a wave packs pixels 64 chunk .. 64 chunk + 63 of one row into words 2 chunk, 2 chunk + 1.
// A pixel past the row's end votes 0, so the tail word's unused bits are zero; NaN > threshold is false.
__global__ __launch_bounds__(kBlock) void occupancy_pack_kernel(const float *alpha, int64_t rows, int32_t width, int32_t channels, int32_t channel,
                                                                float threshold, int32_t chunks, int32_t words, uint32_t *bits)
{
    const int64_t wave = int64_t(blockIdx.x) * kWaves + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (wave >= rows * chunks) return;                      // wave-uniform
    const int64_t row = wave / chunks;
    const int32_t chunk = int32_t(wave - row * chunks);
    const int32_t x = chunk * 64 + lane;
    bool on = false;
    if (x < width) on = alpha[(row * width + x) * channels + channel] > threshold;
    const unsigned long long vote = __ballot(on);
    if (lane == 0) {
        uint32_t *dst = bits + row * words + 2 * chunk;
        dst[0] = uint32_t(vote);
        if (2 * chunk + 1 < words) dst[1] = uint32_t(vote >> 32);
    }
}

// Voxel v = (i G + j) G + k, centre lo + (index + 0.5) step per axis (double, rounded to float32 once).  Inside view b iff
// clip_3 > 0, |clip_0 / clip_3| < 1, |clip_1 / clip_3| < 1 and the pixel's bit is set; a comparison with a NaN is false.  The
// pixel index is formed only after |ndc| < 1 holds, which puts (ndc + 1) 0.5 size in [0, size]: it needs no lower clamp and
// min() takes care of the upper end, so no read leaves the bit image whatever the matrices hold.
__global__ __launch_bounds__(kBlock) void hull_carve_kernel(const uint32_t *__restrict__ bits, const float *__restrict__ mvp, int64_t batch, int32_t height,
                                                            int32_t width, int32_t words, int32_t grid, double lo, double step, uint8_t *__restrict__ hull)
{
    const int32_t n = grid * grid * grid;                   // <= 2^27
    const int32_t v = int32_t(blockIdx.x) * kBlock + threadIdx.x;
    bool inside = v < n;
    const int32_t vv = inside ? v : 0;
    const int32_t i = vv / (grid * grid), r = vv - i * grid * grid, j = r / grid, k = r - j * grid;
    const float x = float(lo + (double(i) + 0.5) * step), y = float(lo + (double(j) + 0.5) * step), z = float(lo + (double(k) + 0.5) * step);
    const float fw = float(width), fh = float(height);
    for (int64_t b = 0; b < batch; ++b) {
        if (!__any(inside)) break;
        const float *m = mvp + b * 16;
        const float c0 = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
        const float c1 = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
        const float c3 = ((m[12] * x + m[13] * y) + m[14] * z) + m[15];
        bool in = false;
        if (inside && c3 > 0.f) {
            const float nx = c0 / c3, ny = c1 / c3;
            if (fabsf(nx) < 1.f && fabsf(ny) < 1.f) {
                const int32_t px = min(width - 1, int32_t(floorf(((nx + 1.f) * 0.5f) * fw)));
                const int32_t py = min(height - 1, int32_t(floorf(((ny + 1.f) * 0.5f) * fh)));
                in = (bits[(b * height + py) * words + (px >> 5)] >> (px & 31)) & 1u;
            }
        }
        inside = in;
    }
    if (v < n) hull[v] = inside ? 1 : 0;
}

// One pass of the separable transform.  A workgroup owns `np` <= kEdtLines whole lines: line p of tile (outer, first) starts at
// outer so + (first + p) sp and steps by sa along the axis.  axis_fast (the pass along the contiguous axis: sa = 1, sp = G) makes
// the axis the fast index of the staging order, otherwise (sp = 1) the line index is: either way consecutive lanes touch
// consecutive addresses and element e of the tile sits at LDS word e.  FIRST reads the mask (f = 0 where it is false, the
// sentinel elsewhere) and reports a false voxel through *status; the later passes do nothing while *status is 0.
// The search walks outwards from a and stops at the first distance whose square alone reaches the best value so far: exact.
template <bool FIRST>
__global__ __launch_bounds__(kBlock) void edt_pass_kernel(const void *__restrict__ in, int32_t *__restrict__ out, int32_t grid, int32_t n_par, int32_t tiles_per_outer,
                                                          int64_t so, int64_t sp, int64_t sa, int32_t axis_fast, int32_t *status)
{
    extern __shared__ int32_t line[];
    if (!FIRST && *status == 0) return;                     // uniform: no false voxel anywhere
    const int32_t outer = int32_t(blockIdx.x) / tiles_per_outer, first = (int32_t(blockIdx.x) - outer * tiles_per_outer) * kEdtLines;
    const int32_t np = min(kEdtLines, n_par - first), count = grid * np;
    const int64_t base = outer * so + first * sp;
    bool found = false;
    for (int32_t e = threadIdx.x; e < count; e += kBlock) {
        const int32_t a = axis_fast ? e % grid : e / np, p = axis_fast ? e / grid : e % np;
        const int64_t at = base + a * sa + p * sp;
        if (FIRST) {
            const bool set = static_cast<const uint8_t *>(in)[at] != 0;
            found |= !set;
            line[e] = set ? kEdtSentinel : 0;
        } else {
            line[e] = static_cast<const int32_t *>(in)[at];
        }
    }
    if (FIRST) {
        if (__any(found) && (threadIdx.x & 63) == 0) atomicOr(status, 1);
    }
    __syncthreads();
    for (int32_t e = threadIdx.x; e < count; e += kBlock) {
        const int32_t a = axis_fast ? e % grid : e / np, p = axis_fast ? e / grid : e % np;
        const int32_t stride = axis_fast ? 1 : np, origin = axis_fast ? p * grid : p;
        int32_t best = line[origin + a * stride];
        for (int32_t d = 1; d < grid; ++d) {
            const int32_t dd = d * d;
            if (dd >= best) break;
            if (a - d >= 0) best = min(best, line[origin + (a - d) * stride] + dd);
            if (a + d < grid) best = min(best, line[origin + (a + d) * stride] + dd);
        }
        out[base + a * sa + p * sp] = best;
    }
}

// Launch t of the cover.  keys[t - 1] holds the maximum launch t - 1 found (0: none).  It stops the sequence when no voxel was
// left, q == 0 or q hs2 < m2: this launch returns at once and leaves keys[t] at 0, which stops launch t + 1 the same way.
// Otherwise (k, q) becomes record t - 1, every voxel with D2(v, k) <= q s2 is cleared, and -- unless this is the last launch --
// the maximum over what is left goes to keys[t].  Integer max: the result does not depend on the order of the atomics.
__global__ __launch_bounds__(kBlock) void greedy_cover_kernel(const int32_t *__restrict__ d2, uint8_t *__restrict__ uncovered, int32_t grid, int32_t t,
                                                              int32_t n_spheres, double s2, double hs2, double m2, unsigned long long *keys,
                                                              int32_t *flat_out, int32_t *q_out, int32_t *count_out)
{
    __shared__ unsigned long long wave_best[kWaves];
    const int32_t n = grid * grid * grid;
    const bool apply = t > 0, find = t < n_spheres;
    int32_t ci = 0, cj = 0, ck = 0;
    double limit = 0.0;
    if (apply) {
        const unsigned long long key = keys[t - 1];
        const int32_t q = int32_t(uint32_t(key >> 32));
        if (key == 0 || q <= 0 || double(q) * hs2 < m2) return;            // uniform
        const int32_t flat = int32_t(0xFFFFFFFFu - uint32_t(key));
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            flat_out[t - 1] = flat;
            q_out[t - 1] = q;
            *count_out = t;
        }
        ci = flat / (grid * grid);
        cj = (flat - ci * grid * grid) / grid;
        ck = flat - (ci * grid + cj) * grid;
        limit = double(q) * s2;
    }
    unsigned long long best = 0;
    for (int32_t v = int32_t(blockIdx.x) * kBlock + threadIdx.x; v < n; v += int32_t(gridDim.x) * kBlock) {
        if (!uncovered[v]) continue;
        if (apply) {
            const int32_t i = v / (grid * grid), r = v - i * grid * grid, j = r / grid, k = r - j * grid;
            const int32_t dist2 = (i - ci) * (i - ci) + (j - cj) * (j - cj) + (k - ck) * (k - ck);
            if (double(dist2) <= limit) {
                uncovered[v] = 0;
                continue;
            }
        }
        if (find) {
            const unsigned long long key = (static_cast<unsigned long long>(uint32_t(d2[v])) << 32) | (0xFFFFFFFFu - uint32_t(v));
            best = best > key ? best : key;
        }
    }
    if (!find) return;                                                     // uniform
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long other = __shfl_xor(best, off, 64);
        best = best > other ? best : other;
    }
    if ((threadIdx.x & 63) == 0) wave_best[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kWaves; ++w) best = best > wave_best[w] ? best : wave_best[w];
        if (best != 0) atomicMax(&keys[t], best);
    }
}

unsigned blocks_for(int64_t n, int per_block) { return unsigned((n + per_block - 1) / per_block); }

}  // namespace

hipError_t launch_hull_carve(const float *alpha, int64_t batch, int32_t height, int32_t width, int32_t channels, int32_t channel, float threshold,
                             const float *mvp, int32_t grid, double lo, double step, uint32_t *bits, uint8_t *hull, hipStream_t stream)
{
    const int32_t words = (width + 31) / 32, chunks = (width + 63) / 64;
    const int64_t rows = batch * height;
    if (rows > 0 && chunks > 0)
        occupancy_pack_kernel<<<blocks_for(rows * chunks, kWaves), kBlock, 0, stream>>>(alpha, rows, width, channels, channel, threshold, chunks, words, bits);
    const int64_t n = int64_t(grid) * grid * grid;
    hull_carve_kernel<<<blocks_for(n, kBlock), kBlock, 0, stream>>>(bits, mvp, batch, height, width, words, grid, lo, step, hull);
    return hipGetLastError();
}

hipError_t launch_edt_squared(const uint8_t *mask, int32_t grid, int32_t *workspace, int32_t *d2, int32_t *status, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t), stream);
    if (e != hipSuccess) return e;
    const int64_t g = grid, plane = g * g;
    const size_t lds = size_t(kEdtLines) * grid * sizeof(int32_t);
    const int32_t plane_tiles = int32_t(blocks_for(plane, kEdtLines)), row_tiles = int32_t(blocks_for(g, kEdtLines));
    // along k (contiguous): lines (i, j) at (i G + j) G;  along j: lines (i, k) at i G^2 + k;  along i: lines (j, k) at j G + k
    edt_pass_kernel<true><<<plane_tiles, kBlock, lds, stream>>>(mask, d2, grid, int32_t(plane), plane_tiles, 0, g, 1, 1, status);
    edt_pass_kernel<false><<<unsigned(grid) * row_tiles, kBlock, lds, stream>>>(d2, workspace, grid, grid, row_tiles, plane, 1, g, 0, status);
    edt_pass_kernel<false><<<plane_tiles, kBlock, lds, stream>>>(workspace, d2, grid, int32_t(plane), plane_tiles, 0, 1, plane, 0, status);
    return hipGetLastError();
}

hipError_t launch_greedy_cover(const uint8_t *hull, const int32_t *d2, int32_t grid, int32_t n_spheres, double s2, double hs2, double m2,
                               unsigned long long *keys, uint8_t *uncovered, int32_t *flat_out, int32_t *q_out, int32_t *count_out, hipStream_t stream)
{
    const int64_t n = int64_t(grid) * grid * grid;
    hipError_t e = hipMemsetAsync(count_out, 0, sizeof(int32_t), stream);
    if (e == hipSuccess) e = hipMemsetAsync(keys, 0, sizeof(unsigned long long) * (size_t(n_spheres) + 1), stream);
    if (e == hipSuccess && uncovered != hull) e = hipMemcpyAsync(uncovered, hull, size_t(n), hipMemcpyDeviceToDevice, stream);
    if (e != hipSuccess) return e;
    const unsigned blocks = unsigned(n < int64_t(kCoverBlocks) * kBlock ? blocks_for(n, kBlock) : kCoverBlocks);
    for (int32_t t = 0; t <= n_spheres && n_spheres > 0; ++t)
        greedy_cover_kernel<<<blocks, kBlock, 0, stream>>>(d2, uncovered, grid, t, n_spheres, s2, hs2, m2, keys, flat_out, q_out, count_out);
    return hipGetLastError();
}

}  // namespace tsamd
