// gfx950 kernels of the multiresolution hash-grid encoding (grid.h; semantics: tests/hashgrid_oracle.py).
//
//   grid_encode_kernel               forward, one lane per (point, level), the level the slow grid dimension (as tiny-cuda-nn's
//                                    kernel_grid): the waves in flight read one level's table, which stays in L2 / the MALL
//   grid_backward_params_lds_kernel  dL/dparams of the coarse levels whose table fits in LDS (level 0: 32 KB, level 1: 110 KB at
//                                    F = 2): a few workgroups per CU accumulate with LDS float atomics over a grid-stride
//                                    loop, then add the table into global memory with contiguous 256-B atomic wave-instructions
//   grid_backward_params_kernel      dL/dparams of the other levels: one global_atomic_add_f32 per feature, after the lanes of
//                                    a wave that hit the same entry with the same corner (neighbouring pixels in one cell)
//                                    summed their adds on chip (backward_params_point: one body for both atomic kernels,
//                                    which differ in where the add lands)
//   grid_backward_x_kernel           dL/dx, one lane per point looping over the levels: plain stores, bitwise repeatable
//   grid_sorted_*_kernel             the second route to dL/dparams (launch_grid_encode_backward_sorted), every level alike:
//                                    (entry, source) records, a stable radix sort by entry, a segmented sum; no float atomics
//   grid_plan_pack_kernel,           the third route (launch_grid_plan_build / launch_grid_encode_backward_planned): the sorted
//   grid_planned_*_kernel            route's sort done once for a frozen point set, its low record words kept as the plan; a
//                                    backward is then the sorted route's segmented sum (one device body for both) and fold over
//                                    the stored order, every level of a chunk in one launch
//
// What the routes share is written once: segment_sums (the run scan of all three), sort_records (the radix-sort driver of the
// sorted backward and the plan build, over sort_buffers' typed view of the workspace), grid_chunk (grid.h: a chunk's points,
// records, tiles and waves) and with_features (n_features -> the template argument F of every launch_* entry point).
//
// The forward and dL/dx are bitwise deterministic (fixed summation order).  dL/dparams has three routes: the default one is a
// float-atomic sum and may differ in the last bits from run to run (tiny-cuda-nn's does too); the sorted one adds every entry's
// contributions in a fixed order and is bitwise repeatable, and the planned one gives the sorted one's bits (contracts: grid.h).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "grid.h"

namespace tsamd {
namespace {

constexpr int kBlock = 256;
constexpr int kLdsBlock = 1024;
constexpr uint32_t kInvalid = 0xffffffffu;

template <int F>
__device__ __forceinline__ void load_feat(const float *p, float (&v)[F])
{
    if constexpr (F == 1) {
        v[0] = p[0];
    } else if constexpr (F == 2) {
        const float2 t = *reinterpret_cast<const float2 *>(p);
        v[0] = t.x;
        v[1] = t.y;
    } else {
#pragma unroll
        for (int k = 0; k < F; k += 4) {
            const float4 t = *reinterpret_cast<const float4 *>(p + k);
            v[k] = t.x;
            v[k + 1] = t.y;
            v[k + 2] = t.z;
            v[k + 3] = t.w;
        }
    }
}

template <int F>
__device__ __forceinline__ void store_feat(float *p, const float (&v)[F])
{
    if constexpr (F == 1) {
        p[0] = v[0];
    } else if constexpr (F == 2) {
        *reinterpret_cast<float2 *>(p) = make_float2(v[0], v[1]);
    } else {
#pragma unroll
        for (int k = 0; k < F; k += 4) *reinterpret_cast<float4 *>(p + k) = make_float4(v[k], v[k + 1], v[k + 2], v[k + 3]);
    }
}

// pos = fmaf(scale, x, 0.5f); cell = (uint32)(int)floorf(pos); frac = pos - floorf(pos) (no clamping: a negative cell wraps)
struct Cell {
    uint32_t c[3];
    float f[3];
};

__device__ __forceinline__ Cell cell_of(const float (&x)[3], float scale)
{
    Cell cl;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float pos = fmaf(scale, x[d], 0.5f);
        const float fl = floorf(pos);
        cl.c[d] = uint32_t(int(fl));
        cl.f[d] = pos - fl;
    }
    return cl;
}

// tiny-cuda-nn grid_index: dense stride index or the coherent prime hash, uint32 wrap-around, then % entries
__device__ __forceinline__ uint32_t corner_index(const Cell &cl, int corner, uint32_t res, uint32_t entries, bool hashed)
{
    const uint32_t x = cl.c[0] + (corner & 1), y = cl.c[1] + ((corner >> 1) & 1), z = cl.c[2] + ((corner >> 2) & 1);
    const uint32_t i = hashed ? (x ^ (y * 2654435761u) ^ (z * 805459861u)) : (x + y * res + z * (res * res));
    return (entries & (entries - 1)) == 0 ? (i & (entries - 1)) : (i % entries);
}

__device__ __forceinline__ float corner_weight(const Cell &cl, int corner)
{
    const float wx = (corner & 1) ? cl.f[0] : 1.0f - cl.f[0];
    const float wy = (corner & 2) ? cl.f[1] : 1.0f - cl.f[1];
    const float wz = (corner & 4) ? cl.f[2] : 1.0f - cl.f[2];
    return wx * wy * wz;
}

__device__ __forceinline__ void load_point(const float *x, int64_t i, float (&p)[3])
{
    p[0] = x[3 * i];
    p[1] = x[3 * i + 1];
    p[2] = x[3 * i + 2];
}

// Sums v over the run of consecutive lanes holding the same key: the run's first lane then holds the run's sum.  Every lane of
// the wave must call it (inactive lanes pass kInvalid and zeros).  Hillis-Steele suffix scan restricted to the run; skipped (one
// ballot) when no two neighbouring lanes share a key.  The one run scan of all three routes to dL/dparams: the "same bits"
// contract of grid.h rests on it.
struct Runs {
    unsigned long long heads;       // the runs' first lanes
    bool head;                      // this lane is one of them
};

template <int F>
__device__ __forceinline__ Runs segment_sums(uint32_t key, float (&v)[F])
{
    const int lane = __lane_id();
    const uint32_t prev = __shfl_up(key, 1);
    const bool head = lane == 0 || prev != key;
    const unsigned long long heads = __ballot(head);
    if (heads == ~0ull) return {heads, true};
    const unsigned long long rest = lane == 63 ? 0ull : (heads >> (lane + 1));
    const int end = rest ? lane + __ffsll(static_cast<long long>(rest)) - 1 : 63;   // last lane of this lane's run
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
        for (int f = 0; f < F; ++f) {
            const float o = __shfl_down(v[f], d);
            if (lane + d <= end) v[f] += o;
        }
    }
    return {heads, head};
}

template <int F>
__global__ __launch_bounds__(kBlock) void grid_encode_kernel(const float *__restrict__ x, int64_t n, const float *__restrict__ params,
                                                             GridLevels lv, float *__restrict__ out)
{
    const int l = blockIdx.y;
    const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n) return;
    float p[3];
    load_point(x, i, p);
    const Cell cl = cell_of(p, lv.scale[l]);
    const uint32_t res = lv.res[l], entries = lv.entries[l];
    const bool hashed = lv.hashed[l] != 0;
    const float *table = params + lv.offset[l] * F;
    float acc[F];
#pragma unroll
    for (int f = 0; f < F; ++f) acc[f] = 0.0f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        float v[F];
        load_feat<F>(table + int64_t(corner_index(cl, c, res, entries, hashed)) * F, v);
        const float w = corner_weight(cl, c);
#pragma unroll
        for (int f = 0; f < F; ++f) acc[f] = fmaf(w, v[f], acc[f]);
    }
    store_feat<F>(out + i * (int64_t(lv.n_levels) * F) + int64_t(l) * F, acc);
}

// The atomic route's work for point i of level l: w * g of its 8 corners, summed on chip over the lanes of the wave that hit
// the same entry with the same corner, then one add(table, key, sum) per run (table: the level's slice of grad_params; the LDS
// kernel's add ignores it, its sums land in LDS first).  No early return here or in the callers: every lane of the wave takes
// part in segment_sums, so a lane past the end comes here with valid = false.
template <int F, class Add>
__device__ __forceinline__ void backward_params_point(const float *__restrict__ x, const float *__restrict__ grad_out, float *__restrict__ grad_params,
                                                      const GridLevels &lv, int l, int64_t i, bool valid, const Add &add)
{
    float p[3] = {0.0f, 0.0f, 0.0f}, g[F];
#pragma unroll
    for (int f = 0; f < F; ++f) g[f] = 0.0f;
    if (valid) {
        load_point(x, i, p);
        load_feat<F>(grad_out + i * (int64_t(lv.n_levels) * F) + int64_t(l) * F, g);
    }
    const Cell cl = cell_of(p, lv.scale[l]);
    const uint32_t res = lv.res[l], entries = lv.entries[l];
    const bool hashed = lv.hashed[l] != 0;
    float *table = grad_params + lv.offset[l] * F;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const uint32_t key = valid ? corner_index(cl, c, res, entries, hashed) : kInvalid;
        const float w = corner_weight(cl, c);
        float v[F];
#pragma unroll
        for (int f = 0; f < F; ++f) v[f] = w * g[f];
        if (segment_sums<F>(key, v).head && valid) add(table, key, v);
    }
}

template <int F>
__global__ __launch_bounds__(kBlock) void grid_backward_params_kernel(const float *__restrict__ x, int64_t n, GridLevels lv,
                                                                      const float *__restrict__ grad_out, float *__restrict__ grad_params)
{
    const int l = lv.lds_levels + blockIdx.y;
    const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    backward_params_point<F>(x, grad_out, grad_params, lv, l, i, i < n, [](float *table, uint32_t key, const float (&v)[F]) {
        float *dst = table + int64_t(key) * F;
#pragma unroll
        for (int f = 0; f < F; ++f) atomicAdd(dst + f, v[f]);
    });
}

template <int F>
__global__ __launch_bounds__(kLdsBlock) void grid_backward_params_lds_kernel(const float *__restrict__ x, int64_t n, GridLevels lv, int l,
                                                                             const float *__restrict__ grad_out,
                                                                             float *__restrict__ grad_params)
{
    extern __shared__ float acc[];
    const uint32_t n_floats = lv.entries[l] * F;
    for (uint32_t j = threadIdx.x; j < n_floats; j += kLdsBlock) acc[j] = 0.0f;
    __syncthreads();
    const int64_t stride = int64_t(gridDim.x) * kLdsBlock;
    // the loop bound is the same for the whole wave (n rounded up to the stride's multiple of 64)
    const int64_t n_wave = (n + 63) & ~int64_t(63);
    for (int64_t i = int64_t(blockIdx.x) * kLdsBlock + threadIdx.x; i < n_wave; i += stride)
        backward_params_point<F>(x, grad_out, grad_params, lv, l, i, i < n, [](float *, uint32_t key, const float (&v)[F]) {
#pragma unroll
            for (int f = 0; f < F; ++f) atomicAdd(&acc[key * F + f], v[f]);
        });
    __syncthreads();
    float *dst = grad_params + lv.offset[l] * F;
    for (uint32_t j = threadIdx.x; j < n_floats; j += kLdsBlock) {
        const float v = acc[j];
        if (v != 0.0f) atomicAdd(dst + j, v);
    }
}

template <int F>
__global__ __launch_bounds__(kBlock) void grid_backward_x_kernel(const float *__restrict__ x, int64_t n, const float *__restrict__ params,
                                                                 GridLevels lv, const float *__restrict__ grad_out, float *__restrict__ grad_x)
{
    const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n) return;
    float p[3];
    load_point(x, i, p);
    const float *grow = grad_out + i * (int64_t(lv.n_levels) * F);
    float gx[3] = {0.0f, 0.0f, 0.0f};
    for (int l = 0; l < lv.n_levels; ++l) {
        float g[F];
        load_feat<F>(grow + l * F, g);
        const Cell cl = cell_of(p, lv.scale[l]);
        const uint32_t res = lv.res[l], entries = lv.entries[l];
        const bool hashed = lv.hashed[l] != 0;
        const float *table = params + lv.offset[l] * F;
        float gl[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            float v[F];
            load_feat<F>(table + int64_t(corner_index(cl, c, res, entries, hashed)) * F, v);
            float s = 0.0f;                                       // dL / d(corner weight)
#pragma unroll
            for (int f = 0; f < F; ++f) s = fmaf(v[f], g[f], s);
            const float wx = (c & 1) ? cl.f[0] : 1.0f - cl.f[0];
            const float wy = (c & 2) ? cl.f[1] : 1.0f - cl.f[1];
            const float wz = (c & 4) ? cl.f[2] : 1.0f - cl.f[2];
            gl[0] += ((c & 1) ? s : -s) * wy * wz;
            gl[1] += ((c & 2) ? s : -s) * wx * wz;
            gl[2] += ((c & 4) ? s : -s) * wx * wy;
        }
#pragma unroll
        for (int d = 0; d < 3; ++d) gx[d] = fmaf(gl[d], lv.scale[l], gx[d]);
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) grad_x[3 * i + d] = gx[d];
}

inline unsigned blocks_of(int64_t n) { return unsigned((n + kBlock - 1) / kBlock); }

template <int F>
hipError_t encode_f(const float *x, int64_t n, const float *params, const GridLevels &lv, float *out, hipStream_t stream)
{
    hipLaunchKernelGGL(grid_encode_kernel<F>, dim3(blocks_of(n), lv.n_levels), dim3(kBlock), 0, stream, x, n, params, lv, out);
    return hipGetLastError();
}

template <int F>
hipError_t backward_f(const float *x, int64_t n, const float *params, const GridLevels &lv, const float *grad_out, float *grad_params,
                      float *grad_x, hipStream_t stream)
{
    if (grad_params) {
        for (int l = 0; l < lv.lds_levels; ++l) {
            const int bytes = int(lv.entries[l]) * F * int(sizeof(float));
            if (bytes > 64 * 1024) {                     // (per function and device; always raised to the same cap)
                hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&grid_backward_params_lds_kernel<F>),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, kGridLdsBytes);
                if (e != hipSuccess) return e;
            }
            // about 16 points per lane and at most one workgroup per CU: the table flush stays small against the points
            const int64_t want = (n + int64_t(kLdsBlock) * 16 - 1) / (int64_t(kLdsBlock) * 16);
            const unsigned nblk = unsigned(want < 1 ? 1 : (want > 256 ? 256 : want));
            hipLaunchKernelGGL(grid_backward_params_lds_kernel<F>, dim3(nblk), dim3(kLdsBlock), bytes, stream, x, n, lv, l, grad_out,
                               grad_params);
            hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
        if (lv.n_levels > lv.lds_levels) {
            hipLaunchKernelGGL(grid_backward_params_kernel<F>, dim3(blocks_of(n), lv.n_levels - lv.lds_levels), dim3(kBlock), 0, stream, x,
                               n, lv, grad_out, grad_params);
            hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
    }
    if (grad_x) {
        hipLaunchKernelGGL(grid_backward_x_kernel<F>, dim3(blocks_of(n)), dim3(kBlock), 0, stream, x, n, params, lv, grad_out, grad_x);
        return hipGetLastError();
    }
    return hipSuccess;
}

// ------------------------------------------------------------------------------------------------ the sorted dL/dparams route
// Per chunk of at most kGridSortedChunk points and per level: a key pass writes one record (entry << 32 | 8 * point + corner)
// per (point, corner) and the level's slice of grad_out as a compact array; a stable LSD radix sort (8-bit digits, only the
// bits the level's entry count needs) orders the records by entry; a segmented sum rebuilds w * g per record from the compact
// arrays and adds every entry's run in a fixed order.  No float atomics; the only atomics count digits in LDS.
using Rec = unsigned long long;

constexpr int kSortBlock = 256;
constexpr int kSortWaves = kSortBlock / 64;
constexpr int kSortItems = kGridSortTile / kSortBlock;                 // records per lane of a sort tile
constexpr int kSumSteps = kGridSumRun / 64;
static_assert(kGridSortTile % (8 * kSortBlock) == 0 && kGridSumRun % 64 == 0, "tile / run sizes");

// Exclusive prefix of v over the workgroup's kSortBlock threads in thread order (integer: exact), and the total.
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t *wave_sums, uint32_t &total)
{
    const int lane = __lane_id(), wave = threadIdx.x / 64;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wave_sums[wave] = inc;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kSortWaves; ++w) {
        const uint32_t s = wave_sums[w];
        if (w < wave) before += s;
        total += s;
    }
    __syncthreads();
    return before + inc - v;
}

// One workgroup per sort tile (kGridSortTile records = kGridSortTile / 8 points): records in (point, corner) order, the level's
// grad_out slice compacted into gl, and the tile's histogram of the first digit.  hist is [digit][tile].  kWithG = false (the
// plan build: records only) reads no grad_out and writes no gl.
template <int F, bool kWithG = true>
__global__ __launch_bounds__(kSortBlock) void grid_sorted_key_kernel(const float *__restrict__ x, uint32_t n, GridLevels lv, int l,
                                                                     const float *__restrict__ grad_out, Rec *__restrict__ rec,
                                                                     float *__restrict__ gl, uint32_t *__restrict__ hist, uint32_t n_tiles)
{
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const float scale = lv.scale[l];
    const uint32_t res = lv.res[l], entries = lv.entries[l];
    const bool hashed = lv.hashed[l] != 0;
    const int64_t row = int64_t(lv.n_levels) * F;
#pragma unroll
    for (int r = 0; r < kGridSortTile / (8 * kSortBlock); ++r) {
        const uint32_t i = blockIdx.x * (kGridSortTile / 8) + r * kSortBlock + threadIdx.x;
        if (i >= n) continue;
        float p[3];
        load_point(x, i, p);
        if constexpr (kWithG) {
            float g[F];
            load_feat<F>(grad_out + i * row + int64_t(l) * F, g);
            store_feat<F>(gl + int64_t(i) * F, g);
        }
        const Cell cl = cell_of(p, scale);
        ulonglong2 *dst = reinterpret_cast<ulonglong2 *>(rec + int64_t(i) * 8);
#pragma unroll
        for (int c = 0; c < 8; c += 2) {
            const uint32_t k0 = corner_index(cl, c, res, entries, hashed), k1 = corner_index(cl, c + 1, res, entries, hashed);
            dst[c / 2] = make_ulonglong2((Rec(k0) << 32) | (i * 8 + c), (Rec(k1) << 32) | (i * 8 + c + 1));
            atomicAdd(&h[k0 & 0xff], 1u);
            atomicAdd(&h[k1 & 0xff], 1u);
        }
    }
    __syncthreads();
    hist[threadIdx.x * n_tiles + blockIdx.x] = h[threadIdx.x];
}

// The per-tile digit histogram of a later radix pass.
__global__ __launch_bounds__(kSortBlock) void grid_sorted_hist_kernel(const Rec *__restrict__ rec, uint32_t n_rec, int shift,
                                                                      uint32_t *__restrict__ hist, uint32_t n_tiles)
{
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kSortItems; ++k) {
        const uint32_t pos = blockIdx.x * kGridSortTile + k * kSortBlock + threadIdx.x;
        if (pos < n_rec) atomicAdd(&h[uint32_t(rec[pos] >> (32 + shift)) & 0xff], 1u);
    }
    __syncthreads();
    hist[threadIdx.x * n_tiles + blockIdx.x] = h[threadIdx.x];
}

// One workgroup per digit: its row of tile counts becomes the exclusive prefix inside the digit, tot[digit] the digit's count.
__global__ __launch_bounds__(kSortBlock) void grid_sorted_scan_kernel(uint32_t *__restrict__ hist, uint32_t n_tiles, uint32_t *__restrict__ tot)
{
    __shared__ uint32_t wave_sums[kSortWaves];
    uint32_t *row = hist + blockIdx.x * n_tiles;
    const uint32_t per = (n_tiles + kSortBlock - 1) / kSortBlock;
    const uint32_t b = threadIdx.x * per, e = b + per < n_tiles ? b + per : n_tiles;
    uint32_t s = 0;
    for (uint32_t j = b; j < e; ++j) s += row[j];
    uint32_t total;
    uint32_t run = block_exclusive_scan(s, wave_sums, total);
    for (uint32_t j = b; j < e; ++j) {
        const uint32_t t = row[j];
        row[j] = run;
        run += t;
    }
    if (threadIdx.x == 0) tot[blockIdx.x] = total;
}

// Stable scatter of one radix pass.  Wave w of a tile owns the tile's w-th quarter and walks it 64 records at a time, so
// (tile, wave, step, lane) is the input order.  A record's rank among the records of its digit: the digit's global base (scan
// of tot), the tile's prefix inside the digit (hist), the earlier waves' counts (cnt after phase 2), the wave's earlier steps
// (cnt, advanced by the first lane of each match group) and the lower lanes of its match mask.  Nothing takes an order from
// the return value of an atomic.
__global__ __launch_bounds__(kSortBlock) void grid_sorted_scatter_kernel(const Rec *__restrict__ in, uint32_t n_rec, int shift,
                                                                         const uint32_t *__restrict__ hist, const uint32_t *__restrict__ tot,
                                                                         uint32_t n_tiles, Rec *__restrict__ out)
{
    __shared__ uint32_t cnt[kSortWaves][256];
    __shared__ uint32_t wave_sums[kSortWaves];
    const int lane = __lane_id(), wave = threadIdx.x / 64;
#pragma unroll
    for (int w = 0; w < kSortWaves; ++w) cnt[w][threadIdx.x] = 0;
    uint32_t total;
    const uint32_t digit_base = block_exclusive_scan(tot[threadIdx.x], wave_sums, total);     // (its barriers cover the zeroing)
    const uint32_t wbase = blockIdx.x * kGridSortTile + wave * (kGridSortTile / kSortWaves);
    Rec r[kSortItems];
#pragma unroll
    for (int k = 0; k < kSortItems; ++k) {
        const uint32_t pos = wbase + k * 64 + lane;
        r[k] = pos < n_rec ? in[pos] : ~Rec(0);
        if (pos < n_rec) atomicAdd(&cnt[wave][uint32_t(r[k] >> (32 + shift)) & 0xff], 1u);
    }
    __syncthreads();
    {
        uint32_t run = digit_base + hist[threadIdx.x * n_tiles + blockIdx.x];
#pragma unroll
        for (int w = 0; w < kSortWaves; ++w) {
            const uint32_t t = cnt[w][threadIdx.x];
            cnt[w][threadIdx.x] = run;
            run += t;
        }
    }
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1;
#pragma unroll
    for (int k = 0; k < kSortItems; ++k) {
        const bool valid = wbase + k * 64 + lane < n_rec;
        const uint32_t digit = uint32_t(r[k] >> (32 + shift)) & 0xff;
        unsigned long long mask = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (digit >> b) & 1;
            const unsigned long long m = __ballot(valid && bit);
            mask &= bit ? m : ~m;
        }
        if (valid) {
            const uint32_t base = cnt[wave][digit];
            const uint32_t rank = __popcll(mask & below);
            if (base + rank < n_rec) out[base + rank] = r[k];       // (always true; keeps a broken count from writing outside)
            if (rank == 0) cnt[wave][digit] = base + __popcll(mask);
        }
        __syncthreads();                              // the next step reads what the group leaders stored
    }
}

// Plain load - add - store by the one lane that owns the entry in this launch.
template <int F>
__device__ __forceinline__ void add_entry(float *table, uint32_t key, const float (&v)[F])
{
    float t[F];
    float *dst = table + int64_t(key) * F;
    load_feat<F>(dst, t);
#pragma unroll
    for (int f = 0; f < F; ++f) t[f] += v[f];
    store_feat<F>(dst, t);
}

// Where a lane's record comes from.  A source gives the record's 4-byte `src` (8 * point + corner, kInvalid past the end),
// says whether the record may be followed at all, and names its entry once the point's cell is known.
//   SortedRecords: the 8-byte records of the radix sort; the entry is the record's high word.
//   PlannedRecords: the 4-byte src of a point plan; the entry is rebuilt from the cell, so it is < entries whatever the plan holds.
// g_stride: floats between two points' g vectors (F: a compact level slice; n_levels * F: a row of grad_out).
template <int F>
struct SortedRecords {
    const Rec *rec;
    __device__ __forceinline__ uint32_t read(uint32_t pos, uint32_t n_rec, uint32_t &hi) const
    {
        const Rec r = pos < n_rec ? rec[pos] : ~Rec(0);
        hi = uint32_t(r >> 32);
        return uint32_t(r);
    }
    __device__ __forceinline__ bool follows(uint32_t hi, uint32_t entries) const { return hi < entries; }
    __device__ __forceinline__ uint32_t key(uint32_t hi, const Cell &, int) const { return hi; }
    __device__ __forceinline__ int64_t g_stride() const { return F; }
};

struct PlannedRecords {
    const uint32_t *src;
    uint32_t res, entries;
    bool hashed;
    int64_t stride;
    __device__ __forceinline__ uint32_t read(uint32_t pos, uint32_t n_rec, uint32_t &hi) const
    {
        hi = 0;
        return pos < n_rec ? src[pos] : kInvalid;
    }
    __device__ __forceinline__ bool follows(uint32_t, uint32_t) const { return true; }
    __device__ __forceinline__ uint32_t key(uint32_t, const Cell &cl, int corner) const { return corner_index(cl, corner, res, entries, hashed); }
    __device__ __forceinline__ int64_t g_stride() const { return stride; }
};

// Segmented sum over records in sorted order: one wave per kGridSumRun consecutive records, 64 at a time.  A run of equal keys
// inside a step is summed by segment_sums (a tree fixed by the lane positions); a run that goes on into the next step is
// carried wave-uniformly and added in step order.  A run that lies strictly inside the wave's range is added to the table
// here (no other wave sees its key); the run that starts at the range's first record and the one that ends at its last may
// go on in the neighbouring waves, so they go to pkey / psum ([2 * wave]: first, [2 * wave + 1]: last, kInvalid: none) for
// the fold.  A range that is one single run is its first partial.  The one body of both routes: the same instructions
// on the same values in the same order, whichever source the records come from.
template <int F, class Source>
__device__ __forceinline__ void segmented_sum(const Source &source, uint32_t n_rec, const float *__restrict__ x, const float *__restrict__ gl,
                                              float scale, uint32_t entries, float *__restrict__ table, uint32_t *__restrict__ pkey,
                                              float *__restrict__ psum)
{
    const int lane = __lane_id();
    const uint32_t wave = blockIdx.x * kSortWaves + threadIdx.x / 64;
    const uint32_t wbase = wave * kGridSumRun;
    if (wbase >= n_rec) return;                       // (whole waves only; no workgroup barrier below)
    uint32_t ckey = kInvalid, fkey = kInvalid;        // the open run at the end of the last step; the range's first run once closed
    bool cfirst = false;                              // the open run started at the range's first record
    float csum[F], fsum[F];
#pragma unroll
    for (int f = 0; f < F; ++f) csum[f] = fsum[f] = 0.0f;
    for (int s = 0; s < kSumSteps; ++s) {
        const uint32_t pos = wbase + s * 64 + lane;
        uint32_t key = kInvalid;
        float v[F];
#pragma unroll
        for (int f = 0; f < F; ++f) v[f] = 0.0f;
        uint32_t hi;
        const uint32_t src = source.read(pos, n_rec, hi), i = src >> 3;
        if (source.follows(hi, entries) && src < n_rec) {                 // (a record is followed only while in bounds)
            float p[3], g[F];
            load_point(x, i, p);
            load_feat<F>(gl + int64_t(i) * source.g_stride(), g);
            const Cell cl = cell_of(p, scale);
            key = source.key(hi, cl, int(src & 7));
            const float w = corner_weight(cl, int(src & 7));
#pragma unroll
            for (int f = 0; f < F; ++f) v[f] = w * g[f];
        }
        const unsigned long long heads = segment_sums<F>(key, v).heads;
        const bool head = (heads >> lane) & 1;
        const int last_head = 63 - __clzll(static_cast<long long>(heads));
        const uint32_t key0 = __shfl(key, 0);
        const bool first0 = s == 0 || (ckey == key0 && cfirst);           // lane 0's run started at the range's first record
        if (ckey != kInvalid) {
            if (ckey == key0) {
                if (lane == 0) {
#pragma unroll
                    for (int f = 0; f < F; ++f) v[f] = csum[f] + v[f];
                }
            } else if (cfirst) {
                fkey = ckey;
#pragma unroll
                for (int f = 0; f < F; ++f) fsum[f] = csum[f];
            } else if (lane == 0) {
                add_entry<F>(table, ckey, csum);
            }
        }
        float v0[F], vl[F];
#pragma unroll
        for (int f = 0; f < F; ++f) {
            v0[f] = __shfl(v[f], 0);
            vl[f] = __shfl(v[f], last_head);
        }
        const uint32_t keyl = __shfl(key, last_head);
        if (last_head != 0 && key0 != kInvalid && first0) {               // the first run closes in this step
            fkey = key0;
#pragma unroll
            for (int f = 0; f < F; ++f) fsum[f] = v0[f];
        }
        if (head && lane != last_head && key != kInvalid && !(lane == 0 && first0)) add_entry<F>(table, key, v);
        ckey = keyl;
        cfirst = last_head == 0 && first0;
#pragma unroll
        for (int f = 0; f < F; ++f) csum[f] = vl[f];
    }
    if (ckey != kInvalid && cfirst) {
        fkey = ckey;
        ckey = kInvalid;
#pragma unroll
        for (int f = 0; f < F; ++f) fsum[f] = csum[f];
    }
    if (lane == 0) {
        pkey[2 * wave] = fkey;
        pkey[2 * wave + 1] = ckey;
        store_feat<F>(psum + int64_t(2 * wave) * F, fsum);
        store_feat<F>(psum + int64_t(2 * wave + 1) * F, csum);
    }
}

template <int F>
__global__ __launch_bounds__(kSortBlock) void grid_sorted_sum_kernel(const Rec *__restrict__ rec, uint32_t n_rec, const float *__restrict__ x,
                                                                     const float *__restrict__ gl, float scale, uint32_t entries,
                                                                     float *__restrict__ table, uint32_t *__restrict__ pkey,
                                                                     float *__restrict__ psum)
{
    segmented_sum<F>(SortedRecords<F>{rec}, n_rec, x, gl, scale, entries, table, pkey, psum);
}

// The planned sum: every level of a chunk in one launch (blockIdx.y: the level).  plan: [level][n_rec] src; g: the first
// point's g vector of level 0, g_level floats on to the next level's, g_stride floats on to the next point's; pkey / psum:
// [level][2 * n_waves].
template <int F>
__global__ __launch_bounds__(kSortBlock) void grid_planned_sum_kernel(const uint32_t *__restrict__ plan, uint32_t n_rec,
                                                                      const float *__restrict__ x, const float *__restrict__ g, int64_t g_level,
                                                                      int64_t g_stride, GridLevels lv, float *__restrict__ grad_params,
                                                                      uint32_t *__restrict__ pkey, float *__restrict__ psum, uint32_t n_waves)
{
    const int l = blockIdx.y;
    const uint32_t entries = lv.entries[l];
    const PlannedRecords source{plan + int64_t(l) * n_rec, lv.res[l], entries, lv.hashed[l] != 0, g_stride};
    segmented_sum<F>(source, n_rec, x, g + int64_t(l) * g_level, lv.scale[l], entries, grad_params + lv.offset[l] * F,
                     pkey + int64_t(l) * 2 * n_waves, psum + int64_t(l) * 2 * n_waves * F);
}

// The boundary partials in wave order: the lane of an entry's first partial adds the entry's partials in that order.
template <int F>
__device__ __forceinline__ void fold_partials(const uint32_t *__restrict__ pkey, const float *__restrict__ psum, uint32_t n_part,
                                              float *__restrict__ table)
{
    const uint32_t j = blockIdx.x * kSortBlock + threadIdx.x;
    if (j >= n_part) return;
    const uint32_t key = pkey[j];
    if (key == kInvalid) return;
    if (j > 0) {                                      // (a range's first partial always exists: no two kInvalid in a row)
        uint32_t before = pkey[j - 1];
        if (before == kInvalid && j > 1) before = pkey[j - 2];
        if (before == key) return;
    }
    float sum[F];
    load_feat<F>(psum + int64_t(j) * F, sum);
    for (uint32_t k = j + 1; k < n_part; ++k) {
        const uint32_t other = pkey[k];
        if (other == kInvalid) continue;
        if (other != key) break;
        float t[F];
        load_feat<F>(psum + int64_t(k) * F, t);
#pragma unroll
        for (int f = 0; f < F; ++f) sum[f] += t[f];
    }
    add_entry<F>(table, key, sum);
}

template <int F>
__global__ __launch_bounds__(kSortBlock) void grid_sorted_fold_kernel(const uint32_t *__restrict__ pkey, const float *__restrict__ psum,
                                                                      uint32_t n_part, float *__restrict__ table)
{
    fold_partials<F>(pkey, psum, n_part, table);
}

template <int F>
__global__ __launch_bounds__(kSortBlock) void grid_planned_fold_kernel(const uint32_t *__restrict__ pkey, const float *__restrict__ psum,
                                                                       uint32_t n_part, GridLevels lv, float *__restrict__ grad_params)
{
    const int l = blockIdx.y;
    fold_partials<F>(pkey + int64_t(l) * n_part, psum + int64_t(l) * n_part * F, n_part, grad_params + lv.offset[l] * F);
}

// The low word of every sorted record (8 * point_in_chunk + corner): what a point plan keeps of the sort.
__global__ __launch_bounds__(kSortBlock) void grid_plan_pack_kernel(const Rec *__restrict__ rec, uint32_t n_rec, uint32_t *__restrict__ plan)
{
    const uint32_t pos = blockIdx.x * kSortBlock + threadIdx.x;
    if (pos < n_rec) plan[pos] = uint32_t(rec[pos]);
}

inline int key_bits(uint32_t entries)
{
    int bits = 1;
    while (bits < 32 && (uint64_t(1) << bits) < entries) ++bits;
    return bits;
}

#define TSAMD_GRID_LAUNCHED()                            \
    do {                                                 \
        const hipError_t e_ = hipGetLastError();         \
        if (e_ != hipSuccess) return e_;                 \
    } while (0)

// The sorted route's workspace (grid.h: GridSortedWorkspace) as typed pointers.
struct SortBuffers {
    Rec *rec_a, *rec_b;
    float *gl, *psum;
    uint32_t *hist, *tot, *pkey;
};

inline SortBuffers sort_buffers(void *workspace, const GridSortedWorkspace &ws)
{
    char *base = static_cast<char *>(workspace);
    return {reinterpret_cast<Rec *>(base + ws.rec_a), reinterpret_cast<Rec *>(base + ws.rec_b), reinterpret_cast<float *>(base + ws.gl),
            reinterpret_cast<float *>(base + ws.psum), reinterpret_cast<uint32_t *>(base + ws.hist), reinterpret_cast<uint32_t *>(base + ws.tot),
            reinterpret_cast<uint32_t *>(base + ws.pkey)};
}

// Sorts a level's records by entry, after the key kernel left them in rec_a and the first digit's histogram in hist: one
// stable pass per 8-bit digit of the bits the entry count needs, ping-pong between rec_a and rec_b.  *sorted: the buffer that
// holds the result.
hipError_t sort_records(const GridChunk &ch, uint32_t entries, const SortBuffers &b, hipStream_t stream, Rec **sorted)
{
    Rec *src = b.rec_a, *dst = b.rec_b;
    const int passes = (key_bits(entries) + 7) / 8;
    for (int p = 0; p < passes; ++p) {
        if (p > 0) {
            hipLaunchKernelGGL(grid_sorted_hist_kernel, dim3(ch.tiles), dim3(kSortBlock), 0, stream, src, ch.records, 8 * p, b.hist, ch.tiles);
            TSAMD_GRID_LAUNCHED();
        }
        hipLaunchKernelGGL(grid_sorted_scan_kernel, dim3(256), dim3(kSortBlock), 0, stream, b.hist, ch.tiles, b.tot);
        TSAMD_GRID_LAUNCHED();
        hipLaunchKernelGGL(grid_sorted_scatter_kernel, dim3(ch.tiles), dim3(kSortBlock), 0, stream, src, ch.records, 8 * p, b.hist, b.tot, ch.tiles,
                           dst);
        TSAMD_GRID_LAUNCHED();
        Rec *t = src;
        src = dst;
        dst = t;
    }
    *sorted = src;
    return hipSuccess;
}

template <int F>
hipError_t backward_sorted_f(const float *x, int64_t n, const float *params, const GridLevels &lv, const float *grad_out, float *grad_params,
                             float *grad_x, void *workspace, hipStream_t stream)
{
    if (grad_params) {
        const SortBuffers b = sort_buffers(workspace, grid_sorted_workspace(n, F));
        const int64_t row = int64_t(lv.n_levels) * F;
        for (int64_t first = 0; first < n; first += kGridSortedChunk) {           // chunks in order: part of the summation order
            const GridChunk ch = grid_chunk(n - first);
            const float *xc = x + first * 3, *gc = grad_out + first * row;
            for (int l = 0; l < lv.n_levels; ++l) {
                hipLaunchKernelGGL(grid_sorted_key_kernel<F>, dim3(ch.tiles), dim3(kSortBlock), 0, stream, xc, ch.points, lv, l, gc, b.rec_a, b.gl,
                                   b.hist, ch.tiles);
                TSAMD_GRID_LAUNCHED();
                Rec *sorted = nullptr;
                const hipError_t e = sort_records(ch, lv.entries[l], b, stream, &sorted);
                if (e != hipSuccess) return e;
                float *table = grad_params + lv.offset[l] * F;
                hipLaunchKernelGGL(grid_sorted_sum_kernel<F>, dim3((ch.waves + kSortWaves - 1) / kSortWaves), dim3(kSortBlock), 0, stream, sorted,
                                   ch.records, xc, b.gl, lv.scale[l], lv.entries[l], table, b.pkey, b.psum);
                TSAMD_GRID_LAUNCHED();
                hipLaunchKernelGGL(grid_sorted_fold_kernel<F>, dim3((2 * ch.waves + kSortBlock - 1) / kSortBlock), dim3(kSortBlock), 0, stream, b.pkey,
                                   b.psum, 2 * ch.waves, table);
                TSAMD_GRID_LAUNCHED();
            }
        }
    }
    if (grad_x) {
        hipLaunchKernelGGL(grid_backward_x_kernel<F>, dim3(blocks_of(n)), dim3(kBlock), 0, stream, x, n, params, lv, grad_out, grad_x);
        return hipGetLastError();
    }
    return hipSuccess;
}

// The plan of a frozen point set: per chunk and level, the records sorted as above with only their low word kept, laid out
// [chunk][level][8 * points_in_chunk].  The workspace is the sorted route's.
hipError_t plan_build(const float *x, int64_t n, const GridLevels &lv, int32_t n_features, uint32_t *plan, void *workspace, hipStream_t stream)
{
    const SortBuffers b = sort_buffers(workspace, grid_sorted_workspace(n, n_features));
    for (int64_t first = 0; first < n; first += kGridSortedChunk) {
        const GridChunk ch = grid_chunk(n - first);
        const float *xc = x + first * 3;
        uint32_t *pc = plan + first * 8 * lv.n_levels;
        for (int l = 0; l < lv.n_levels; ++l) {
            hipLaunchKernelGGL((grid_sorted_key_kernel<1, false>), dim3(ch.tiles), dim3(kSortBlock), 0, stream, xc, ch.points, lv, l,
                               static_cast<const float *>(nullptr), b.rec_a, static_cast<float *>(nullptr), b.hist, ch.tiles);
            TSAMD_GRID_LAUNCHED();
            Rec *sorted = nullptr;
            const hipError_t e = sort_records(ch, lv.entries[l], b, stream, &sorted);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(grid_plan_pack_kernel, dim3((ch.records + kSortBlock - 1) / kSortBlock), dim3(kSortBlock), 0, stream, sorted,
                               ch.records, pc + l * ch.records);
            TSAMD_GRID_LAUNCHED();
        }
    }
    return hipSuccess;
}

template <int F>
hipError_t backward_planned_f(const float *x, int64_t n, const GridLevels &lv, const float *grad_out, float *grad_params, const uint32_t *plan,
                              void *workspace, hipStream_t stream)
{
    const GridPlannedWorkspace ws = grid_planned_workspace(n, F, lv.n_levels);
    char *base = static_cast<char *>(workspace);
    uint32_t *pkey = reinterpret_cast<uint32_t *>(base + ws.pkey);
    float *psum = reinterpret_cast<float *>(base + ws.psum);
    const int64_t row = int64_t(lv.n_levels) * F;
    for (int64_t first = 0; first < n; first += kGridSortedChunk) {               // chunks in order: part of the summation order
        const GridChunk ch = grid_chunk(n - first);
        const float *xc = x + first * 3, *gc = grad_out + first * row;
        const uint32_t *pc = plan + first * 8 * lv.n_levels;
        // g is read straight from the rows of grad_out (level l at + l * F, the next point's a row on)
        hipLaunchKernelGGL(grid_planned_sum_kernel<F>, dim3((ch.waves + kSortWaves - 1) / kSortWaves, lv.n_levels), dim3(kSortBlock), 0, stream, pc,
                           ch.records, xc, gc, int64_t(F), row, lv, grad_params, pkey, psum, ch.waves);
        TSAMD_GRID_LAUNCHED();
        hipLaunchKernelGGL(grid_planned_fold_kernel<F>, dim3((2 * ch.waves + kSortBlock - 1) / kSortBlock, lv.n_levels), dim3(kSortBlock), 0, stream,
                           pkey, psum, 2 * ch.waves, lv, grad_params);
        TSAMD_GRID_LAUNCHED();
    }
    return hipSuccess;
}

#undef TSAMD_GRID_LAUNCHED

// Calls fn with n_features as a compile-time constant (fn(std::integral_constant<int, F>{})), for the F the kernels are built for.
template <class Fn>
hipError_t with_features(int32_t n_features, Fn fn)
{
    switch (n_features) {
    case 1: return fn(std::integral_constant<int, 1>{});
    case 2: return fn(std::integral_constant<int, 2>{});
    case 4: return fn(std::integral_constant<int, 4>{});
    case 8: return fn(std::integral_constant<int, 8>{});
    default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_grid_plan_build(const float *x, int64_t n, const GridLevels &lv, int32_t n_features, void *plan, void *workspace,
                                  hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    return plan_build(x, n, lv, n_features, static_cast<uint32_t *>(plan), workspace, stream);
}

hipError_t launch_grid_encode_backward_planned(const float *x, int64_t n, const GridLevels &lv, int32_t n_features, const float *grad_out,
                                               float *grad_params, const void *plan, void *workspace, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    return with_features(n_features, [&](auto f) {
        return backward_planned_f<f()>(x, n, lv, grad_out, grad_params, static_cast<const uint32_t *>(plan), workspace, stream);
    });
}

hipError_t launch_grid_encode_backward_sorted(const float *x, int64_t n, const float *params, const GridLevels &lv, int32_t n_features,
                                              const float *grad_out, float *grad_params, float *grad_x, void *workspace, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    return with_features(n_features,
                         [&](auto f) { return backward_sorted_f<f()>(x, n, params, lv, grad_out, grad_params, grad_x, workspace, stream); });
}

hipError_t launch_grid_encode(const float *x, int64_t n, const float *params, const GridLevels &lv, int32_t n_features, float *out,
                              hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    return with_features(n_features, [&](auto f) { return encode_f<f()>(x, n, params, lv, out, stream); });
}

hipError_t launch_grid_encode_backward(const float *x, int64_t n, const float *params, const GridLevels &lv, int32_t n_features,
                                       const float *grad_out, float *grad_params, float *grad_x, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    return with_features(n_features, [&](auto f) { return backward_f<f()>(x, n, params, lv, grad_out, grad_params, grad_x, stream); });
}

}  // namespace tsamd
