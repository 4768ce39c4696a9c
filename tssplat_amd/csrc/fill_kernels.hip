// gfx950 kernels of the merge's flood fill: connected components of the inside / outside nodes of a field under the extraction's
// own connectivity (the seven owned Kuhn edges of a node and their reverses), and the fill of enclosed cavities / the removal of
// islands built on them.  Semantics: tests/fill_oracle.py.  Integers only: no flag of _build.SOURCE_FLAGS applies.
//   cc_tile_kernel        one workgroup per tile of 4 x 8 x 16 nodes (k fastest): runs of equal bits along k from one ballot, then a
//                         union-find of the tile's nodes in LDS over the owned edges that stay in the tile and are not implied by
//                         others (needed_edges), then label = the flat index of the tile-local root
//   cc_merge_kernel       one lane per node on a tile's upper faces: lock-free unions, with path compression, on the global labels
//                         over the owned edges that leave the tile through a face, an edge or a corner and are not implied
//   cc_flatten_kernel     label[n] = root(n), so that label[label[n]] == label[n]
//   fill_mark_kernel      one lane per node of the grid's six faces: marks the labels of outside border nodes (the exterior)
//   fill_cavities_kernel  every outside node whose label is unmarked becomes +inf; counts cavities and their nodes
//   fill_count_kernel     nodes per solid label, one integer atomic per run of equal labels in the 512 nodes of a wave
//   fill_best_kernel      the largest solid component by the key (count, smaller label) through a 64-bit integer atomicMax
//   fill_outer_kernel     every solid node outside that component becomes outside; counts islands and their nodes
// A link always points at a smaller or equal index (label[x] <= x), a union only ever lowers a root's link with an integer
// atomicMin, so the root of a component is its smallest flat index whatever the execution order: the labels are bitwise
// repeatable.  Every walk and every retry loop is bounded (see find_root / unite); a loop that runs out of its bound raises the
// status word and leaves.  No workgroup waits for another.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "merge.h"

namespace tsamd {

namespace {

constexpr int kBlock = 256;
constexpr int kTileI = 4, kTileJ = 8, kTileK = 16;            // powers of two: the masks below rely on it
constexpr int kTile = kTileI * kTileJ * kTileK;              // 512 nodes, one lane each
constexpr int kCountChunks = 8;                              // chunks of 64 nodes per wave of fill_count_kernel

__device__ inline bool inside_of(float v, float level) { return v > level; }          // a NaN is outside

// The root of x: follows links, which strictly decrease, until label[r] == r.  `budget` is the number of links the caller may
// still follow; -1 when it runs out (the caller raises the status word).
__device__ inline int32_t find_root(int32_t *L, int32_t x, int32_t &budget)
{
    for (;;) {
        const int32_t p = __atomic_load_n(L + x, __ATOMIC_RELAXED);
        if (p == x) return x;
        if (--budget < 0) return -1;
        x = p;
    }
}

// Lock-free union of the trees of a and b: link the larger root to the smaller with atomicMin; if the larger one stopped being
// a root meanwhile (the atomic returns another value), go on with what it pointed at, which lies in the same tree.
// Bound: over the whole call a and b only ever decrease, every followed link and every retry lowers one of them strictly, and
// both start below n: at most 2 n links and n retries.  budget = 3 n + 8.
// kCompress: a start node that is not its root is linked to the root found (atomicMin again: the root is an ancestor, so no link
// of the tree is lost, and a node that has stopped being a root never becomes one again), which keeps later walks short.
template <bool kCompress>
__device__ inline void unite(int32_t *L, int32_t a, int32_t b, int32_t budget, int32_t *status)
{
    for (;;) {
        const int32_t a0 = a, b0 = b;
        a = find_root(L, a, budget);
        b = a < 0 ? -1 : find_root(L, b, budget);
        if (a < 0 || b < 0 || --budget < 0) {
            atomicMax(status, kFillStatusUnionBound);
            return;
        }
        if (kCompress) {
            if (a != a0 && __atomic_load_n(L + a0, __ATOMIC_RELAXED) > a) atomicMin(L + a0, a);
            if (b != b0 && __atomic_load_n(L + b0, __ATOMIC_RELAXED) > b) atomicMin(L + b0, b);
        }
        if (a == b) return;
        if (a < b) {
            const int32_t s = a;
            a = b;
            b = s;
        }
        const int32_t old = atomicMin(L + a, b);
        if (old == a) return;
        a = old;
    }
}

// The owned edges of a node v that have to be united, as a mask over m = 4 di + 2 dj + dk; the others follow from edges of lower
// order (fewer set bits of m first, then a smaller k), so leaving them out loses no connection:
//   - a diagonal edge v -> v + m is implied when an intermediate corner v + s, s a non-zero proper submask of m, has v's inside bit:
//     v -> v + s and v + s -> v + m are both edges (of fewer bits) between nodes of that bit;
//   - the edges (1, 0, 0) and (0, 1, 0) are implied when the same edge one node back along k exists and both of its ends continue
//     to the ends of this one: three edges of the same number of bits with a smaller k.
// same: bit m set iff node v + m exists for the caller and has v's inside bit (m in 1 .. 7).  back: bits 0, 4, 2 set iff the node one
// step back along k from v, v + (1, 0, 0), v + (0, 1, 0) exists for the caller and has v's inside bit.
// In a uniform region this leaves the (0, 0, 1) edge and one edge per row towards the next row and the next plane.
__device__ inline uint32_t needed_edges(uint32_t same, uint32_t back)
{
    uint32_t need = same & 0x16u;                                                      // one bit set: 1, 2, 4
    if ((same & 0x08u) && !(same & 0x06u)) need |= 0x08u;                              // 3 = 1 | 2: neither corner 1 nor corner 2
    if ((same & 0x20u) && !(same & 0x12u)) need |= 0x20u;                              // 5 = 1 | 4
    if ((same & 0x40u) && !(same & 0x14u)) need |= 0x40u;                              // 6 = 2 | 4
    if ((same & 0xFEu) == 0x80u) need |= 0x80u;                                         // 7: none of the corners 1 .. 6
    if ((back & 1u) && (back & 0x10u)) need &= ~0x10u;
    if ((back & 1u) && (back & 0x04u)) need &= ~0x04u;
    return need;
}

__global__ __launch_bounds__(kTile) void cc_tile_kernel(const float *__restrict__ field, int32_t grid, float level, int32_t *__restrict__ label,
                                                        int32_t *status)
{
    __shared__ int32_t s_label[kTile];
    __shared__ uint8_t s_inside[kTile];                       // 0 outside, 1 inside, 2 beyond the grid
    const int t = threadIdx.x;
    const int lk = t & (kTileK - 1), lj = (t / kTileK) & (kTileJ - 1), li = t / (kTileK * kTileJ);
    const int32_t i = int32_t(blockIdx.z) * kTileI + li, j = int32_t(blockIdx.y) * kTileJ + lj, k = int32_t(blockIdx.x) * kTileK + lk;
    const bool valid = i < grid && j < grid && k < grid;
    const int32_t flat = (i * grid + j) * grid + k;           // < 2^27 when valid, never used otherwise
    const uint8_t mine = valid ? (inside_of(field[flat], level) ? 1 : 0) : 2;
    s_inside[t] = mine;
    // the (0, 0, 1) edges without a union: a row of the tile is 16 consecutive lanes of one wave, and a node starts at the first
    // node of its run of equal bits
    const int before = __shfl_up(int(mine), 1);
    const uint64_t starts = __ballot(lk == 0 || before != int(mine));
    const uint32_t row_starts = uint32_t(starts >> (t & 48)) & ((2u << lk) - 1u);        // bit 0 is always set
    s_label[t] = t - lk + (31 - __clz(row_starts));
    __syncthreads();
    if (valid) {
        uint32_t same = 0;
        for (int m = 1; m < 8; ++m) {
            const int di = (m >> 2) & 1, dj = (m >> 1) & 1, dk = m & 1;
            if (li + di < kTileI && lj + dj < kTileJ && lk + dk < kTileK && s_inside[t + (di * kTileJ + dj) * kTileK + dk] == mine) same |= 1u << m;
        }
        uint32_t back = 0;
        if (lk > 0) {
            if (s_inside[t - 1] == mine) back |= 0x01u;
            if (li + 1 < kTileI && s_inside[t + kTileJ * kTileK - 1] == mine) back |= 0x10u;
            if (lj + 1 < kTileJ && s_inside[t + kTileK - 1] == mine) back |= 0x04u;
        }
        const uint32_t need = needed_edges(same, back) & ~0x02u;                        // (0, 0, 1): the runs
        for (int m = 2; m < 8; ++m) {
            if (!((need >> m) & 1u)) continue;
            const int di = (m >> 2) & 1, dj = (m >> 1) & 1, dk = m & 1;
            unite<false>(s_label, t, t + (di * kTileJ + dj) * kTileK + dk, 3 * kTile + 8, status);
        }
    }
    __syncthreads();
    if (valid) {
        int32_t budget = kTile;
        int32_t r = find_root(s_label, t, budget);
        if (r < 0) {
            atomicMax(status, kFillStatusFindBound);
            r = t;
        }
        // the local order (li, lj, lk) is the order of the flat indices, so the tile-local root is the tile-local minimum
        const int rk = r & (kTileK - 1), rj = (r / kTileK) & (kTileJ - 1), ri = r / (kTileK * kTileJ);
        label[flat] = ((i - li + ri) * grid + (j - lj + rj)) * grid + (k - lk + rk);
    }
}

__global__ __launch_bounds__(kBlock) void cc_merge_kernel(const float *__restrict__ field, int32_t grid, float level, int32_t *label, int32_t *status)
{
    const int32_t n = grid * grid * grid;
    const int32_t v = int32_t(blockIdx.x) * kBlock + threadIdx.x;
    if (v >= n) return;
    const int32_t i = v / (grid * grid), r = v - i * grid * grid, j = r / grid, k = r - j * grid;
    const bool top_i = (i & (kTileI - 1)) == kTileI - 1, top_j = (j & (kTileJ - 1)) == kTileJ - 1, top_k = (k & (kTileK - 1)) == kTileK - 1;
    if (!(top_i || top_j || top_k)) return;                    // every owned edge stays in the tile
    const bool mine = inside_of(field[v], level);
    uint32_t same = 0, cross = 0;
    for (int m = 1; m < 8; ++m) {
        const int di = (m >> 2) & 1, dj = (m >> 1) & 1, dk = m & 1;
        if (i + di >= grid || j + dj >= grid || k + dk >= grid) continue;
        if ((di && top_i) || (dj && top_j) || (dk && top_k)) cross |= 1u << m;        // the others: the tile kernel has done them
        if (inside_of(field[v + (di * grid + dj) * grid + dk], level) == mine) same |= 1u << m;
    }
    uint32_t back = 0;
    if (k > 0 && (same & 0x14u) != 0 && inside_of(field[v - 1], level) == mine) {
        back = 0x01u;
        if ((same & 0x10u) && inside_of(field[v + grid * grid - 1], level) == mine) back |= 0x10u;
        if ((same & 0x04u) && inside_of(field[v + grid - 1], level) == mine) back |= 0x04u;
    }
    uint32_t need = needed_edges(same, back) & cross;
    if (need == 0) return;
    const int32_t mine_label = __atomic_load_n(label + v, __ATOMIC_RELAXED);           // an ancestor of v: as good a start as v
    if (need & 0x02u) {
        // The (0, 0, 1) edge through a tile's k face is implied by the same edge one node back along j (or i) when the tile kernel
        // has already joined both of its ends to the ends of this one: equal links mean one tree.  (What is relied on is a finished
        // launch and an edge of this kind at a smaller (i, j), so nothing goes round in a circle.)
        const int32_t other = __atomic_load_n(label + v + 1, __ATOMIC_RELAXED);
        for (int axis = 0; axis < 2; ++axis) {
            const int32_t step = axis == 0 ? grid : grid * grid;
            if ((axis == 0 ? j : i) == 0) continue;
            if (inside_of(field[v - step], level) == mine && inside_of(field[v - step + 1], level) == mine &&
                __atomic_load_n(label + v - step, __ATOMIC_RELAXED) == mine_label && __atomic_load_n(label + v - step + 1, __ATOMIC_RELAXED) == other) {
                need &= ~0x02u;
                break;
            }
        }
    }
    for (int m = 1; m < 8; ++m) {
        if (!((need >> m) & 1u)) continue;
        const int di = (m >> 2) & 1, dj = (m >> 1) & 1, dk = m & 1;
        const int32_t other = __atomic_load_n(label + v + (di * grid + dj) * grid + dk, __ATOMIC_RELAXED);
        if (other != mine_label) unite<true>(label, mine_label, other, 3 * n + 8, status);
    }
}

__global__ __launch_bounds__(kBlock) void cc_flatten_kernel(int32_t *label, int32_t n, int32_t *status)
{
    const int32_t v = int32_t(blockIdx.x) * kBlock + threadIdx.x;
    if (v >= n) return;
    int32_t budget = n;
    const int32_t t = __atomic_load_n(label + v, __ATOMIC_RELAXED);                    // the tile-local root, for all but that root itself
    const int32_t r = find_root(label, t, budget);
    if (r < 0) {
        atomicMax(status, kFillStatusFindBound);
        return;
    }
    // No union runs any more, so roots are final.  A concurrent lane reads either an old link or the root: both lie on the path to
    // the same root.  The tile's nodes share t: the first lane through shortens the walk of the others.
    if (t != r && __atomic_load_n(label + t, __ATOMIC_RELAXED) != r) __atomic_store_n(label + t, r, __ATOMIC_RELAXED);
    if (t != r) __atomic_store_n(label + v, r, __ATOMIC_RELAXED);
}

// ---- the fill ----
__global__ __launch_bounds__(kBlock) void fill_mark_kernel(const float *__restrict__ field, int32_t grid, float level, const int32_t *__restrict__ label,
                                                           int32_t *mark)
{
    const int32_t e = int32_t(blockIdx.x) * kBlock + threadIdx.x;                     // < 6 * 512^2
    if (e >= 6 * grid * grid) return;
    const int32_t face = e / (grid * grid), r = e - face * grid * grid, a = r / grid, b = r - a * grid;
    const int32_t fixed = (face & 1) ? grid - 1 : 0;
    const int32_t i = face < 2 ? fixed : a, j = face < 2 ? a : (face < 4 ? fixed : b), k = face < 4 ? b : fixed;
    const int32_t v = (i * grid + j) * grid + k;
    if (inside_of(field[v], level)) return;
    const int32_t l = label[v];
    if (l >= 0 && l <= v) mark[l] = 1;                         // (a label is a flat index <= the node's own)
}

__device__ inline void add_count(int32_t *dst, bool flag)
{
    const uint64_t votes = __ballot(flag);
    if (votes != 0 && (threadIdx.x & 63) == 0) atomicAdd(dst, int32_t(__popcll(votes)));
}

__global__ __launch_bounds__(kBlock) void fill_cavities_kernel(const float *__restrict__ field, int32_t grid, float level,
                                                               const int32_t *__restrict__ label, const int32_t *__restrict__ mark,
                                                               float *__restrict__ out, int32_t *stats)
{
    const int32_t n = grid * grid * grid;
    const int32_t v = int32_t(blockIdx.x) * kBlock + threadIdx.x;
    bool cavity = false, root = false;
    if (v < n) {
        const float f = field[v];
        int32_t l = label[v];
        if (l < 0 || l > v) l = v;
        cavity = !inside_of(f, level) && mark[l] == 0;
        root = cavity && l == v;
        out[v] = cavity ? __uint_as_float(0x7F800000u) : f;    // +inf; an unchanged node keeps its bits
    }
    add_count(stats + kFillStatCavities, root);
    add_count(stats + kFillStatCavityNodes, cavity);
}

__global__ __launch_bounds__(kBlock) void fill_count_kernel(const float *__restrict__ solid_field, int32_t n, float level, const int32_t *__restrict__ label,
                                                            int32_t *count)
{
    // A wave walks kCountChunks chunks of 64 nodes and keeps one (label, nodes) pair, wave-uniform, which it adds to the counts only
    // when another label turns up: one atomic per run of equal labels, not per node -- most solid nodes share one label.
    const int lane = threadIdx.x & 63;
    const int64_t wave_base = (int64_t(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6)) * (64 * kCountChunks);
    int32_t held_label = -1, held = 0;
    for (int chunk = 0; chunk < kCountChunks; ++chunk) {
        const int64_t v = wave_base + chunk * 64 + lane;
        int32_t l = 0;
        bool solid = false;
        if (v < n) {
            l = label[v];
            solid = inside_of(solid_field[v], level) && l >= 0 && l <= v;
        }
        // each round retires the leader's lane at least: 64 rounds at most
        uint64_t todo = __ballot(solid);
        for (int round = 0; round < 64 && todo != 0; ++round) {
            const int32_t l0 = __shfl(l, __ffsll((unsigned long long)todo) - 1);
            const uint64_t same = __ballot(solid && l == l0) & todo;
            if (l0 != held_label) {
                if (held > 0 && lane == 0) atomicAdd(count + held_label, held);
                held_label = l0;
                held = 0;
            }
            held += int32_t(__popcll(same));
            todo &= ~same;
        }
    }
    if (held > 0 && lane == 0) atomicAdd(count + held_label, held);
}

__global__ __launch_bounds__(kBlock) void fill_best_kernel(const float *__restrict__ solid_field, int32_t n, float level, const int32_t *__restrict__ label,
                                                           const int32_t *__restrict__ count, unsigned long long *best)
{
    const int32_t v = int32_t(blockIdx.x) * kBlock + threadIdx.x;
    if (v >= n || label[v] != v || !inside_of(solid_field[v], level)) return;
    // count first, then the smaller label; > 0 for every solid root
    atomicMax(best, (unsigned long long)(uint32_t(count[v])) << 32 | uint32_t(0x7FFFFFFF - v));
}

__global__ __launch_bounds__(kBlock) void fill_outer_kernel(const float *__restrict__ field, int32_t grid, float level, const int32_t *__restrict__ label,
                                                            const unsigned long long *__restrict__ best, float *out, int32_t *stats)
{
    const int32_t n = grid * grid * grid;
    const int32_t v = int32_t(blockIdx.x) * kBlock + threadIdx.x;
    bool island = false, root = false;
    if (v < n) {
        const unsigned long long key = *best;
        const int32_t keep_label = key ? 0x7FFFFFFF - int32_t(uint32_t(key)) : -1;
        const bool solid = inside_of(out[v], level);
        const int32_t l = label[v];
        const bool keep = solid && l == keep_label;
        island = solid && !keep;
        root = island && l == v;
        const float f = field[v];
        // the inside bit as it was: the value as it was, bit for bit (a cavity inside a dropped island is outside again)
        out[v] = keep == inside_of(f, level) ? f : __uint_as_float(keep ? 0x7F800000u : 0xFF800000u);
    }
    add_count(stats + kFillStatIslands, root);
    add_count(stats + kFillStatIslandNodes, island);
}

unsigned blocks_for(int64_t n, int per_block) { return unsigned((n + per_block - 1) / per_block); }

// label <- the components of `field`; status is raised, never cleared
hipError_t enqueue_components(const float *field, int32_t grid, float level, int32_t *label, int32_t *status, hipStream_t stream)
{
    const int32_t n = grid * grid * grid;
    cc_tile_kernel<<<dim3(blocks_for(grid, kTileK), blocks_for(grid, kTileJ), blocks_for(grid, kTileI)), kTile, 0, stream>>>(field, grid, level, label, status);
    cc_merge_kernel<<<blocks_for(n, kBlock), kBlock, 0, stream>>>(field, grid, level, label, status);
    cc_flatten_kernel<<<blocks_for(n, kBlock), kBlock, 0, stream>>>(label, n, status);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_grid_components(const float *field, int32_t grid, float level, int32_t *label, int32_t *status, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t), stream);
    if (e != hipSuccess) return e;
    return enqueue_components(field, grid, level, label, status, stream);
}

hipError_t launch_field_fill(const float *field, int32_t grid, float level, int32_t mode, int32_t *workspace, float *out, int32_t *stats,
                             hipStream_t stream)
{
    const int32_t n = grid * grid * grid;
    int32_t *label = workspace, *aux = workspace + n;
    unsigned long long *best = reinterpret_cast<unsigned long long *>(workspace + 2 * int64_t(n));      // 8 n bytes in: aligned
    hipError_t e = hipMemsetAsync(stats, 0, kFillStats * sizeof(int32_t), stream);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(aux, 0, (size_t(n) + 2) * sizeof(int32_t), stream)) != hipSuccess) return e;         // the marks and the key
    if ((e = enqueue_components(field, grid, level, label, stats + kFillStatStatus, stream)) != hipSuccess) return e;
    fill_mark_kernel<<<blocks_for(6 * int64_t(grid) * grid, kBlock), kBlock, 0, stream>>>(field, grid, level, label, aux);
    fill_cavities_kernel<<<blocks_for(n, kBlock), kBlock, 0, stream>>>(field, grid, level, label, aux, out, stats);
    if (mode == kFillOuter) {
        // the second labelling: of the solid mask, which is the inside bit of the field just written
        if ((e = hipMemsetAsync(aux, 0, size_t(n) * sizeof(int32_t), stream)) != hipSuccess) return e;
        if ((e = enqueue_components(out, grid, level, label, stats + kFillStatStatus, stream)) != hipSuccess) return e;
        fill_count_kernel<<<blocks_for(n, kBlock * kCountChunks), kBlock, 0, stream>>>(out, n, level, label, aux);
        fill_best_kernel<<<blocks_for(n, kBlock), kBlock, 0, stream>>>(out, n, level, label, aux, best);
        fill_outer_kernel<<<blocks_for(n, kBlock), kBlock, 0, stream>>>(field, grid, level, label, best, out, stats);
    }
    return hipGetLastError();
}

}  // namespace tsamd
