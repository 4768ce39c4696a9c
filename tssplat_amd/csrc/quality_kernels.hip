// gfx950 kernels of the mesh-quality stage: the exact self-intersection search and the topology under it.
//   quality_prepare_kernel     one lane per triangle: the snap to the 2^20 lattice, validity and degeneracy, the packed corners and
//                              box, the Morton key of the box centre, and the float64 shape record
//   quality_tile_boxes_kernel  one workgroup per tile of kQualityTile triangles: the tile's lattice box (integer LDS atomics)
//   quality_pairs_kernel       brute force over pairs i < j.  A workgroup holds kQualityBlock triangles i, one per lane, and streams
//                              the boxes of the triangles j through LDS in tiles of kQualityTile, read at a wave-uniform address.
//                              The reject is j > i and box overlap on the lattice (closed intervals), on the packed words.  A wave
//                              appends its survivors to its own queue in LDS (a ballot and a prefix count: no atomics, no barrier)
//                              and evaluates 64 of them with all 64 lanes whenever 64 are there; what is left is evaluated after
//                              the last tile.  Only tiles with some j > i are visited; with tile boxes, a tile that no wave's box
//                              overlaps is not loaded and a wave whose box misses the tile's does not scan it.
//   quality_finish_kernel      one lane per triangle: crossing, invalid and degenerate faces; the pair list's length
//   quality_edges_kernel       one lane per half-edge: the undirected and the directed key, the vertex pair, the referenced marks
//   quality_fan_pairs_kernel   one lane per sorted key: where it equals the one before, the two corner pairs that edge joins
//   union_init / hook / compress   union-find by hooking a root to the lower index (atomicMin) and pointer jumping
// Semantics: tests/quality_oracle.py.  Every result is an integer except the shape record, whose float64 operations are rounded
// one by one (-ffp-contract=off, _build.py).
//
// Magnitudes of orient(a, b, c, d) = det(b - a, c - a, d - a) on lattice points in 0 .. 2^20 - 1: differences are below 2^20 in
// magnitude, 2 x 2 minors (a difference of two products) below 2^41, each of the three terms minor x difference below 2^61, their
// sum below 3 2^61 < 2^63: int64 never overflows.  The kernel evaluates the determinant as (u x v) . w, the oracle as
// u . (v x w): the same integer, since neither overflows.
//
// Packed words: a lattice point is x | y << 21 | z << 42, 20 bits per field and one guard bit above each.  A box is two words,
// the minimum corner and the maximum corner with the three guard bits set, so that a <= b on all three fields is one 64-bit
// subtraction: the guard bit of a field of (b | guards) - a survives iff that field of b is >= that of a, and no field borrows
// from the next.  A triangle that is not valid or is degenerate has the box (2^20 - 1, 0) and the corner word ~0: the reject
// passes it at most for a box that spans the whole cube, and the evaluation drops it before anything is counted.
//
// Bounds: every loop runs over the triangles, a tile or the queue; a full queue is drained by the wave that filled it, nothing
// waits for another wave.  j < n_triangles for every queue entry, and a lane past the last triangle holds the empty box and ~0.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "quality.h"

namespace tsamd {

namespace {

constexpr int kBlock = 256;
constexpr int kQ = kQualityBlock, kK = kQualityTile, kQueue = kQualityQueue, kWaves = kQ / 64;
constexpr uint64_t kGuards = (1ull << 20) | (1ull << 41) | (1ull << 62);
constexpr uint64_t kFieldMask = 0xFFFFFull;
constexpr uint64_t kEmptyMin = kFieldMask | (kFieldMask << 21) | (kFieldMask << 42), kEmptyMax = kGuards;
constexpr uint64_t kNoCorner = ~0ull;
constexpr long long kNoKey = 0x7FFFFFFFFFFFFFFFll;
static_assert(kQ % 64 == 0 && kK % kQ == 0 && kQueue >= 128, "a wave appends up to 64 entries to fewer than 64");

struct I3 {
    int32_t x, y, z;
};

__device__ inline uint64_t pack(int32_t x, int32_t y, int32_t z) { return uint64_t(uint32_t(x)) | (uint64_t(uint32_t(y)) << 21) | (uint64_t(uint32_t(z)) << 42); }
__device__ inline I3 unpack(uint64_t w) { return I3{int32_t(w & kFieldMask), int32_t((w >> 21) & kFieldMask), int32_t((w >> 42) & kFieldMask)}; }
__device__ inline I3 sub(I3 a, I3 b) { return I3{a.x - b.x, a.y - b.y, a.z - b.z}; }

// closed intervals overlap on all three axes
__device__ inline bool boxes_overlap(uint64_t min_a, uint64_t max_a, uint64_t min_b, uint64_t max_b)
{
    return (((max_b - min_a) & (max_a - min_b)) & kGuards) == kGuards;
}

struct L3 {
    int64_t x, y, z;
};
__device__ inline L3 cross(I3 u, I3 v)
{
    return L3{int64_t(u.y) * v.z - int64_t(u.z) * v.y, int64_t(u.z) * v.x - int64_t(u.x) * v.z, int64_t(u.x) * v.y - int64_t(u.y) * v.x};
}
__device__ inline int64_t dot(L3 n, I3 d) { return n.x * d.x + n.y * d.y + n.z * d.z; }
__device__ inline bool opposite(int64_t s, int64_t t) { return (s > 0 && t < 0) || (s < 0 && t > 0); }

// the segment p q, known to straddle the plane of a b c strictly, passes strictly inside the triangle
__device__ inline bool inside_edges(I3 p, I3 q, I3 a, I3 b, I3 c)
{
    const I3 d = sub(q, p), pa = sub(a, p), pb = sub(b, p), pc = sub(c, p);
    const int64_t o1 = dot(cross(d, pa), pb), o2 = dot(cross(d, pb), pc), o3 = dot(cross(d, pc), pa);
    return (o1 > 0 && o2 > 0 && o3 > 0) || (o1 < 0 && o2 < 0 && o3 < 0);
}

__device__ inline bool triangles_cross(const uint64_t (&wa)[3], const uint64_t (&wb)[3])
{
    const I3 a0 = unpack(wa[0]), a1 = unpack(wa[1]), a2 = unpack(wa[2]), b0 = unpack(wb[0]), b1 = unpack(wb[1]), b2 = unpack(wb[2]);
    const L3 na = cross(sub(a1, a0), sub(a2, a0)), nb = cross(sub(b1, b0), sub(b2, b0));
    const int64_t sb0 = dot(na, sub(b0, a0)), sb1 = dot(na, sub(b1, a0)), sb2 = dot(na, sub(b2, a0));
    const int64_t sa0 = dot(nb, sub(a0, b0)), sa1 = dot(nb, sub(a1, b0)), sa2 = dot(nb, sub(a2, b0));
    bool hit = false;
    if (opposite(sb0, sb1)) hit = hit || inside_edges(b0, b1, a0, a1, a2);
    if (opposite(sb1, sb2)) hit = hit || inside_edges(b1, b2, a0, a1, a2);
    if (opposite(sb2, sb0)) hit = hit || inside_edges(b2, b0, a0, a1, a2);
    if (opposite(sa0, sa1)) hit = hit || inside_edges(a0, a1, b0, b1, b2);
    if (opposite(sa1, sa2)) hit = hit || inside_edges(a1, a2, b0, b1, b2);
    if (opposite(sa2, sa0)) hit = hit || inside_edges(a2, a0, b0, b1, b2);
    return hit;
}

// 20 bits spread to every third bit
__device__ inline uint64_t spread3(uint64_t x)
{
    x &= 0xFFFFFull;
    x = (x | (x << 32)) & 0x001F00000000FFFFull;
    x = (x | (x << 16)) & 0x001F0000FF0000FFull;
    x = (x | (x << 8)) & 0x100F00F00F00F00Full;
    x = (x | (x << 4)) & 0x10C30C30C30C30C3ull;
    x = (x | (x << 2)) & 0x1249249249249249ull;
    return x;
}

__device__ inline double dot3(double x, double y, double z) { return (x * x + y * y) + z * z; }

__global__ __launch_bounds__(kBlock) void quality_prepare_kernel(const float *__restrict__ v, int64_t n_vertices, const int32_t *__restrict__ faces,
                                                                 int64_t n_triangles, double lo, double g, uint64_t *__restrict__ corners,
                                                                 uint64_t *__restrict__ boxes, uint8_t *__restrict__ state, double *__restrict__ shape,
                                                                 long long *__restrict__ morton)
{
    const int64_t t = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (t >= n_triangles) return;
    int64_t idx[3];
    bool ok = true;
    for (int c = 0; c < 3; ++c) {
        idx[c] = faces[t * 3 + c];
        ok = ok && idx[c] >= 0 && idx[c] < n_vertices;
    }
    double p[3][3];
    int32_t X[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float x = ok ? v[idx[c] * 3 + k] : 0.0f;      // nothing is read through a bad index
            p[c][k] = double(x);
            const double s = floor((p[c][k] - lo) * g + 0.5);
            const bool in = (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u && s >= 0.0 && s <= double(kQualityLattice - 1);
            X[c][k] = in ? int32_t(s) : 0;
            ok = ok && in;                                      // (a later corner of a bad triangle reads vertex idx, which is in range, or nothing)
        }
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    double rec[4] = {nan, nan, nan, nan};
    uint8_t st = kQualityInvalid;
    uint64_t w[3] = {kNoCorner, kNoCorner, kNoCorner}, bmin = kEmptyMin, bmax = kEmptyMax;
    long long key = kNoKey;
    if (ok) {
        const double ux = p[1][0] - p[0][0], uy = p[1][1] - p[0][1], uz = p[1][2] - p[0][2];
        const double vx = p[2][0] - p[0][0], vy = p[2][1] - p[0][1], vz = p[2][2] - p[0][2];
        rec[0] = dot3(ux, uy, uz);
        rec[1] = dot3(p[2][0] - p[1][0], p[2][1] - p[1][1], p[2][2] - p[1][2]);
        rec[2] = dot3(p[0][0] - p[2][0], p[0][1] - p[2][1], p[0][2] - p[2][2]);
        rec[3] = dot3(uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx);
        const I3 a{X[0][0], X[0][1], X[0][2]}, b{X[1][0], X[1][1], X[1][2]}, c{X[2][0], X[2][1], X[2][2]};
        const L3 n = cross(sub(b, a), sub(c, a));
        st = (n.x == 0 && n.y == 0 && n.z == 0) ? kQualityDegenerate : kQualityValid;
        if (st == kQualityValid) {
            const int32_t x0 = min(a.x, min(b.x, c.x)), y0 = min(a.y, min(b.y, c.y)), z0 = min(a.z, min(b.z, c.z));
            const int32_t x1 = max(a.x, max(b.x, c.x)), y1 = max(a.y, max(b.y, c.y)), z1 = max(a.z, max(b.z, c.z));
            w[0] = pack(a.x, a.y, a.z);
            w[1] = pack(b.x, b.y, b.z);
            w[2] = pack(c.x, c.y, c.z);
            bmin = pack(x0, y0, z0);
            bmax = pack(x1, y1, z1) | kGuards;
            key = (long long)(spread3(uint64_t((x0 + x1) >> 1)) | (spread3(uint64_t((y0 + y1) >> 1)) << 1) | (spread3(uint64_t((z0 + z1) >> 1)) << 2));
        }
    }
    for (int c = 0; c < 3; ++c) corners[t * 3 + c] = w[c];
    boxes[t * 2] = bmin;
    boxes[t * 2 + 1] = bmax;
    state[t] = st;
    for (int k = 0; k < 4; ++k) shape[t * 4 + k] = rec[k];
    morton[t] = key;
}

// LDS integer min / max of the three fields of box words; identity: the empty box
__device__ inline void lds_box_reset(int32_t *b)
{
    b[0] = b[1] = b[2] = kQualityLattice - 1;
    b[3] = b[4] = b[5] = 0;
}
__device__ inline void lds_box_add(int32_t *b, uint64_t bmin, uint64_t bmax)
{
    const I3 lo = unpack(bmin), hi = unpack(bmax);
    atomicMin(b + 0, lo.x);
    atomicMin(b + 1, lo.y);
    atomicMin(b + 2, lo.z);
    atomicMax(b + 3, hi.x);
    atomicMax(b + 4, hi.y);
    atomicMax(b + 5, hi.z);
}

__global__ __launch_bounds__(kBlock) void quality_tile_boxes_kernel(const uint64_t *__restrict__ boxes, int64_t n_triangles, uint64_t *__restrict__ tile_boxes)
{
    __shared__ int32_t s_box[6];
    if (threadIdx.x == 0) lds_box_reset(s_box);
    __syncthreads();
    const int64_t base = int64_t(blockIdx.x) * kK;
    for (int32_t jj = threadIdx.x; jj < kK; jj += kBlock) {
        const int64_t j = base + jj;
        if (j < n_triangles) lds_box_add(s_box, boxes[j * 2], boxes[j * 2 + 1]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        tile_boxes[int64_t(blockIdx.x) * 2] = pack(s_box[0], s_box[1], s_box[2]);
        tile_boxes[int64_t(blockIdx.x) * 2 + 1] = pack(s_box[3], s_box[4], s_box[5]) | kGuards;
    }
}

// stats words (include/tssplat_amd.h: TSAMD_QUALITY_*)
constexpr int kStatPairs = 0, kStatFaces = 1, kStatInvalid = 2, kStatDegenerate = 3, kStatBox = 4, kStatListed = 5, kStatTiles = 6;

__global__ __launch_bounds__(kQ) void quality_pairs_kernel(const uint64_t *__restrict__ corners, const uint64_t *__restrict__ boxes, int64_t n_triangles,
                                                           const uint64_t *__restrict__ tile_boxes, int64_t tiles_per_chunk, int64_t max_pairs,
                                                           int32_t *crossings, unsigned long long *pairs, unsigned long long *stats)
{
    __shared__ uint64_t s_min[kK], s_max[kK];
    __shared__ uint64_t s_corner[kQ * 3];
    __shared__ uint64_t s_queue[kWaves][kQueue];
    __shared__ int32_t s_wave_box[kWaves][6];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t i0 = int64_t(blockIdx.x) * kQ, i = i0 + tid;
    uint64_t min_i = kEmptyMin, max_i = kEmptyMax;
    if (i < n_triangles) {
        min_i = boxes[i * 2];
        max_i = boxes[i * 2 + 1];
    }
    for (int c = 0; c < 3; ++c) s_corner[tid * 3 + c] = i < n_triangles ? corners[i * 3 + c] : kNoCorner;
    if (lane == 0) lds_box_reset(s_wave_box[wave]);
    __syncthreads();
    if (tile_boxes) lds_box_add(s_wave_box[wave], min_i, max_i);
    __syncthreads();
    uint64_t wave_min[kWaves], wave_max[kWaves];
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        wave_min[w] = pack(s_wave_box[w][0], s_wave_box[w][1], s_wave_box[w][2]);
        wave_max[w] = pack(s_wave_box[w][3], s_wave_box[w][4], s_wave_box[w][5]) | kGuards;
    }
    const int64_t n_tiles = (n_triangles + kK - 1) / kK;
    int64_t tile_lo = (i0 + 1) / kK;                                           // the tile of the first j above the block's first i
    int64_t tile_hi = (int64_t(blockIdx.y) + 1) * tiles_per_chunk;
    if (tile_lo < int64_t(blockIdx.y) * tiles_per_chunk) tile_lo = int64_t(blockIdx.y) * tiles_per_chunk;
    if (tile_hi > n_tiles) tile_hi = n_tiles;
    uint64_t *queue = s_queue[wave];
    int32_t queued = 0;                                                        // wave-uniform, < 64 between steps
    unsigned long long box_pairs = 0, visited = 0;

    // one queue entry: the block's triangle li and the triangle j
    auto evaluate = [&](uint64_t entry) {
        const int32_t li = int32_t(entry >> 32);
        const int64_t j = int64_t(entry & 0xFFFFFFFFull);
        const uint64_t wa[3] = {s_corner[li * 3], s_corner[li * 3 + 1], s_corner[li * 3 + 2]};
        const uint64_t wb[3] = {corners[j * 3], corners[j * 3 + 1], corners[j * 3 + 2]};
        if (wa[0] == kNoCorner || wb[0] == kNoCorner) return;
        ++box_pairs;
        if (!triangles_cross(wa, wb)) return;
        const int64_t gi = i0 + li;
        atomicAdd(crossings + gi, 1);
        atomicAdd(crossings + j, 1);
        const unsigned long long slot = atomicAdd(stats + kStatPairs, 1ull);
        if (slot < (unsigned long long)max_pairs) pairs[slot] = ((unsigned long long)gi << 32) | (unsigned long long)j;
    };

    for (int64_t tile = tile_lo; tile < tile_hi; ++tile) {
        bool mine = true, any = true;
        if (tile_boxes) {
            const uint64_t tmin = tile_boxes[tile * 2], tmax = tile_boxes[tile * 2 + 1];
            any = false;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) {
                const bool o = boxes_overlap(wave_min[w], wave_max[w], tmin, tmax);
                any = any || o;
                if (w == wave) mine = o;
            }
        }
        if (!any) continue;                                                    // workgroup-uniform: the same words in every lane
        if (tid == 0) ++visited;
        const int64_t base = tile * kK;
        __syncthreads();                                                       // the previous tile has been read by every wave
        for (int32_t jj = tid; jj < kK; jj += kQ) {
            const int64_t j = base + jj;
            s_min[jj] = j < n_triangles ? boxes[j * 2] : kEmptyMin;
            s_max[jj] = j < n_triangles ? boxes[j * 2 + 1] : kEmptyMax;
        }
        __syncthreads();
        if (!mine) continue;                                                   // wave-uniform; the barriers above are passed by all
        const int32_t count = int32_t(n_triangles - base < kK ? n_triangles - base : kK);
        for (int32_t jj = 0; jj < count; ++jj) {
            const int64_t j = base + jj;
            const bool pass = j > i && boxes_overlap(min_i, max_i, s_min[jj], s_max[jj]);
            const unsigned long long ballot = __ballot(pass);
            if (ballot == 0) continue;                                         // wave-uniform
            if (pass) queue[queued + __popcll(ballot & ((1ull << lane) - 1ull))] = (uint64_t(uint32_t(tid)) << 32) | uint64_t(j);
            queued += __popcll(ballot);                                        // <= 63 + 64 < kQueue
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (queued >= 64) {                                                // drain: the last 64 entries, one per lane
                queued -= 64;
                evaluate(queue[queued + lane]);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
    if (lane < queued) evaluate(queue[lane]);
    if (box_pairs) atomicAdd(stats + kStatBox, box_pairs);
    if (visited) atomicAdd(stats + kStatTiles, visited);
}

__global__ __launch_bounds__(kBlock) void quality_finish_kernel(const int32_t *__restrict__ crossings, const uint8_t *__restrict__ state, int64_t n_triangles,
                                                                int64_t max_pairs, unsigned long long *stats)
{
    const int64_t t = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    const bool in = t < n_triangles;
    const uint8_t st = in ? state[t] : kQualityValid;
    const unsigned long long crossing = __ballot(in && crossings[t] > 0), invalid = __ballot(in && st == kQualityInvalid),
                             degenerate = __ballot(in && st == kQualityDegenerate);
    if ((threadIdx.x & 63) == 0) {
        if (crossing) atomicAdd(stats + kStatFaces, (unsigned long long)__popcll(crossing));
        if (invalid) atomicAdd(stats + kStatInvalid, (unsigned long long)__popcll(invalid));
        if (degenerate) atomicAdd(stats + kStatDegenerate, (unsigned long long)__popcll(degenerate));
    }
    if (t == 0) {                                                              // the pair kernel has finished: its counter is final
        const unsigned long long found = stats[kStatPairs];
        stats[kStatListed] = found < (unsigned long long)max_pairs ? found : (unsigned long long)max_pairs;
    }
}

__global__ __launch_bounds__(kBlock) void quality_edges_kernel(const int32_t *__restrict__ faces, const uint8_t *__restrict__ state, int64_t n_triangles,
                                                               int64_t n_vertices, long long *__restrict__ und_keys, long long *__restrict__ dir_keys,
                                                               int32_t *__restrict__ vertex_pairs, uint8_t *referenced)
{
    const int64_t h = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (h >= 3 * n_triangles) return;
    const int64_t t = h / 3;
    const int k = int(h - 3 * t);
    const int64_t a = faces[t * 3 + k], b = faces[t * 3 + (k + 1) % 3], c = faces[t * 3 + (k + 2) % 3];
    const bool valid = state[t] != kQualityInvalid && a >= 0 && a < n_vertices && b >= 0 && b < n_vertices && c >= 0 && c < n_vertices;
    und_keys[h] = valid ? (long long)(((a < b ? a : b) << 32) | (a < b ? b : a)) : kNoKey;
    dir_keys[h] = valid ? (long long)((a << 32) | b) : kNoKey;
    vertex_pairs[h * 2] = valid ? int32_t(a) : -1;
    vertex_pairs[h * 2 + 1] = valid ? int32_t(b) : -1;
    if (valid) referenced[a] = 1;                                              // every writer stores the same byte
}

__global__ __launch_bounds__(kBlock) void quality_fan_pairs_kernel(const int32_t *__restrict__ faces, int64_t n_triangles, const long long *__restrict__ keys,
                                                                   const long long *__restrict__ order, int32_t *__restrict__ corner_pairs)
{
    const int64_t p = int64_t(blockIdx.x) * kBlock + threadIdx.x, n = 3 * n_triangles;
    if (p >= n) return;
    int32_t out[4] = {-1, -1, -1, -1};
    if (p > 0 && keys[p] == keys[p - 1] && keys[p] != kNoKey) {
        const int64_t h1 = order[p - 1], h2 = order[p];
        if (h1 >= 0 && h1 < n && h2 >= 0 && h2 < n) {                          // a permutation, or nothing is read
            const int64_t t1 = h1 / 3, t2 = h2 / 3;
            const int k1 = int(h1 - 3 * t1), k2 = int(h2 - 3 * t2);
            for (int e = 0; e < 2; ++e) {
                const int64_t c1 = 3 * t1 + (k1 + e) % 3;
                const int64_t c2 = faces[3 * t2 + k2] == faces[c1] ? 3 * t2 + k2 : 3 * t2 + (k2 + 1) % 3;
                out[2 * e] = int32_t(c1);
                out[2 * e + 1] = int32_t(c2);
            }
        }
    }
    for (int q = 0; q < 4; ++q) corner_pairs[p * 4 + q] = out[q];
}

// ---- union-find: label[x] <= x always; a root has label[x] == x; after a compress pass every label is a root ----
__global__ __launch_bounds__(kBlock) void union_init_kernel(int32_t *__restrict__ label, int64_t n)
{
    const int64_t x = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (x < n) label[x] = int32_t(x);
}

// one lane per pair: the higher of the two labels read is hooked to the lower.  A link only ever goes down and only ever joins
// two elements of one component; a link an atomicMin overwrites is found again by its pair in the next round, which the flag asks for
__global__ __launch_bounds__(kBlock) void union_hook_kernel(const int32_t *__restrict__ pairs, int64_t n_pairs, int32_t *label, int64_t n, int32_t *changed)
{
    const int64_t p = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (p >= n_pairs) return;
    const int64_t a = pairs[p * 2], b = pairs[p * 2 + 1];
    if (a < 0 || b < 0 || a >= n || b >= n) return;
    const int32_t ra = __atomic_load_n(label + a, __ATOMIC_RELAXED), rb = __atomic_load_n(label + b, __ATOMIC_RELAXED);
    if (ra == rb) return;
    atomicMin(label + (ra > rb ? ra : rb), ra > rb ? rb : ra);
    *changed = 1;
}

// pointer jumping: links strictly decrease, so a walk ends within n steps; the bound is explicit all the same
__global__ __launch_bounds__(kBlock) void union_compress_kernel(int32_t *label, int64_t n)
{
    const int64_t x = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (x >= n) return;
    int32_t r = __atomic_load_n(label + x, __ATOMIC_RELAXED);
    for (int64_t step = 0; step < n; ++step) {
        const int32_t up = __atomic_load_n(label + r, __ATOMIC_RELAXED);
        if (up == r) break;
        r = up;
    }
    __atomic_store_n(label + x, r, __ATOMIC_RELAXED);
}

inline unsigned blocks_for(int64_t items) { return unsigned((items + kBlock - 1) / kBlock); }

}  // namespace

hipError_t launch_quality_prepare(const float *v, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, double lo, double hi, uint64_t *corners,
                                  uint64_t *boxes, uint8_t *state, double *shape, int64_t *morton, hipStream_t stream)
{
    const double g = double(kQualityLattice - 1) / (hi - lo);
    hipLaunchKernelGGL(quality_prepare_kernel, dim3(blocks_for(n_triangles)), dim3(kBlock), 0, stream, v, n_vertices, faces, n_triangles, lo, g, corners, boxes,
                       state, shape, reinterpret_cast<long long *>(morton));
    return hipGetLastError();
}

hipError_t launch_quality_pairs(const uint64_t *corners, const uint64_t *boxes, const uint8_t *state, int64_t n_triangles, uint64_t *tile_boxes,
                                int64_t max_pairs, int32_t *crossings, int64_t *pairs, int64_t *stats, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(crossings, 0, size_t(n_triangles) * sizeof(int32_t), stream);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(stats, 0, kQualityStats * sizeof(int64_t), stream)) != hipSuccess) return e;
    const int64_t tiles = quality_tiles(n_triangles), blocks = (n_triangles + kQ - 1) / kQ;
    if (tile_boxes) hipLaunchKernelGGL(quality_tile_boxes_kernel, dim3(unsigned(tiles)), dim3(kBlock), 0, stream, boxes, n_triangles, tile_boxes);
    int64_t chunks = (kQualityTargetWorkgroups + blocks - 1) / blocks;
    if (chunks > tiles) chunks = tiles;
    if (chunks > kQualityMaxChunks) chunks = kQualityMaxChunks;
    if (chunks < 1) chunks = 1;
    const int64_t tiles_per_chunk = (tiles + chunks - 1) / chunks;
    auto *st = reinterpret_cast<unsigned long long *>(stats);
    hipLaunchKernelGGL(quality_pairs_kernel, dim3(unsigned(blocks), unsigned(chunks)), dim3(kQ), 0, stream, corners, boxes, n_triangles, tile_boxes,
                       tiles_per_chunk, max_pairs, crossings, reinterpret_cast<unsigned long long *>(pairs), st);
    hipLaunchKernelGGL(quality_finish_kernel, dim3(blocks_for(n_triangles)), dim3(kBlock), 0, stream, crossings, state, n_triangles, max_pairs, st);
    return hipGetLastError();
}

hipError_t launch_quality_edges(const int32_t *faces, const uint8_t *state, int64_t n_triangles, int64_t n_vertices, int64_t *und_keys, int64_t *dir_keys,
                                int32_t *vertex_pairs, uint8_t *referenced, hipStream_t stream)
{
    if (n_vertices > 0) {
        hipError_t e = hipMemsetAsync(referenced, 0, size_t(n_vertices), stream);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(quality_edges_kernel, dim3(blocks_for(3 * n_triangles)), dim3(kBlock), 0, stream, faces, state, n_triangles, n_vertices,
                       reinterpret_cast<long long *>(und_keys), reinterpret_cast<long long *>(dir_keys), vertex_pairs, referenced);
    return hipGetLastError();
}

hipError_t launch_quality_fan_pairs(const int32_t *faces, int64_t n_triangles, const int64_t *sorted_keys, const int64_t *order, int32_t *corner_pairs,
                                    hipStream_t stream)
{
    hipLaunchKernelGGL(quality_fan_pairs_kernel, dim3(blocks_for(3 * n_triangles)), dim3(kBlock), 0, stream, faces, n_triangles,
                       reinterpret_cast<const long long *>(sorted_keys), reinterpret_cast<const long long *>(order), corner_pairs);
    return hipGetLastError();
}

hipError_t launch_quality_union(const int32_t *pairs, int64_t n_pairs, int32_t *labels, int64_t n, int32_t *flag_dev, int64_t round_cap, int32_t *converged,
                                int64_t *rounds_out, hipStream_t stream)
{
    *converged = 0;
    *rounds_out = 0;
    hipLaunchKernelGGL(union_init_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, stream, labels, n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (n_pairs == 0) {
        *converged = 1;
        return hipSuccess;
    }
    for (int64_t round = 0; round < round_cap; ++round) {                      // bounded: past the cap the caller reports an error
        int32_t changed = 0;
        if ((e = hipMemsetAsync(flag_dev, 0, sizeof(int32_t), stream)) != hipSuccess) return e;
        hipLaunchKernelGGL(union_hook_kernel, dim3(blocks_for(n_pairs)), dim3(kBlock), 0, stream, pairs, n_pairs, labels, n, flag_dev);
        hipLaunchKernelGGL(union_compress_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, stream, labels, n);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(&changed, flag_dev, sizeof(int32_t), hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
        if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
        *rounds_out = round + 1;
        if (!changed) {
            *converged = 1;
            return hipSuccess;
        }
    }
    return hipSuccess;
}

}  // namespace tsamd
