// gfx950 kernels of the mesh voxeliser: the integer winding number of a triangle mesh at the nodes of the merge's grid.
//   voxel_deposit_kernel   one lane per (face, ray): the corners on the 2^-10 lattice, the exact int64 area and edge functions, the
//                          clipped box of candidate columns.  A box of at most kVoxelLaneColumns columns is walked by the lane itself
//                          (a loop of that compile-time length); a larger one by the lane's whole wave, 64 columns per trip, one such
//                          face after the other (at most 64 faces, at most G^2 / 64 trips each: both known at launch).  A covered column
//                          gets -sign(area) at slab ceil(x) by an int32 atomicAdd whose result is not used.  blockIdx.y is the ray
//   voxel_walk_kernel      rays along i and j: one lane per column, the lanes of a wave on consecutive k, so every slab is one coalesced
//                          row; eight loads in flight per lane.  Writes w, or the ray's rule bit into the occupancy byte
//   voxel_row_kernel       the ray along k: the column is the contiguous direction, so one wave takes one row of G + 1 slabs, 64 per trip,
//                          with a shuffle prefix sum and a carry.  Writes w, or takes the vote of the three bits and counts the nodes at
//                          which they differ
//   voxel_stats_kernel     the twelve counts: every kernel above adds to one of 64 copies of the record, this one sums them
// Semantics: tests/voxel_oracle.py.  Coverage is integer work; the crossing's float64 operations are rounded one by one
// (-ffp-contract=off, _build.py; IEEE division).  The deposits are integer sums, so neither the order of the atomics nor the split of
// the faces between lanes and waves changes a bit: the results are bitwise repeatable and equal the oracle's.  Nothing is read through
// a bad index; every loop is bounded by a number known at launch.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "voxel.h"

namespace tsamd {

namespace {

constexpr int kBlock = 256;
constexpr int kWave = 64;
constexpr int32_t kS = 1 << kVoxelSubcellBits;
using u64 = unsigned long long;

inline unsigned blocks_for(int64_t n) { return unsigned((n + kBlock - 1) / kBlock); }

struct VoxFace {
    int32_t ab, ac, bb, bc, cb, cc;      // the corners A, B, C on the plane axes b and c, lattice units
    double ra, rb, rc;                   // their ray coordinates, node units
    long long area;
    int32_t b0, c0, nc, cols;            // the candidate columns: cols = nb * nc, column q is (b0 + q / nc, c0 + q % nc)
};

__device__ inline int32_t pick(const int32_t u[3], int axis) { return axis == 0 ? u[0] : (axis == 1 ? u[1] : u[2]); }
__device__ inline double pick(const double u[3], int axis) { return axis == 0 ? u[0] : (axis == 1 ? u[1] : u[2]); }
__device__ inline int32_t min3(int32_t a, int32_t b, int32_t c) { return min(a, min(b, c)); }
__device__ inline int32_t max3(int32_t a, int32_t b, int32_t c) { return max(a, max(b, c)); }

// u = floor(t S + 0.5) and r = t - 0.5 with t = (x - lo) / h; usable iff |u| <= 2^29 on all three axes (a NaN fails the comparison)
__device__ inline bool load_vertex(const float *__restrict__ v, int64_t idx, double lo, double h, int32_t u[3], double r[3])
{
    bool ok = true;
    for (int x = 0; x < 3; ++x) {
        const double t = (double(v[idx * 3 + x]) - lo) / h;
        const double fu = floor(t * double(kS) + 0.5);
        const bool in = fabs(fu) <= double(kVoxelLatticeMax);
        u[x] = in ? int32_t(fu) : 0;
        r[x] = t - 0.5;
        ok = ok && in;
    }
    return ok;
}

__device__ inline bool inner_side(long long e, long long db, long long dc) { return e > 0 || (e == 0 && (db > 0 || (db == 0 && dc > 0))); }

// One candidate column (p, q) of the plane: the three edge functions, the fill rule, the crossing and the deposit.  Returns 1 when covered
__device__ inline int deposit_column(const VoxFace &f, int sg, int32_t p, int32_t q, int32_t G, int axis, int32_t *__restrict__ dep)
{
    const long long Pb = (long long)p * kS + kS / 2, Pc = (long long)q * kS + kS / 2;
    const long long bc_b = f.cb - f.bb, bc_c = f.cc - f.bc, ca_b = f.ab - f.cb, ca_c = f.ac - f.cc, ab_b = f.bb - f.ab, ab_c = f.bc - f.ac;
    const long long e_bc = bc_b * (Pc - f.bc) - bc_c * (Pb - f.bb);
    const long long e_ca = ca_b * (Pc - f.cc) - ca_c * (Pb - f.cb);
    const long long e_ab = ab_b * (Pc - f.ac) - ab_c * (Pb - f.ab);
    if (!(inner_side(sg * e_bc, sg * bc_b, sg * bc_c) && inner_side(sg * e_ca, sg * ca_b, sg * ca_c) && inner_side(sg * e_ab, sg * ab_b, sg * ab_c))) return 0;
    double x = ((double(e_bc) * f.ra + double(e_ca) * f.rb) + double(e_ab) * f.rc) / double(f.area);
    x = ceil(x);
    if (!(x > 0.0)) x = 0.0;
    if (x > double(G)) x = double(G);
    const int64_t s = int64_t(x);
    // axis 0: (slab, j, k); axis 1: (slab, i, k) with p = k and q = i; axis 2: (i, j, slab), rows of G + 1
    const int64_t at = axis == 0 ? (s * G + p) * G + q : (axis == 1 ? (s * G + q) * G + p : (int64_t(p) * G + q) * (G + 1) + s);
    atomicAdd(dep + at, -sg);
    return 1;
}

// The counts go to one of kVoxelStatReplicas copies of the record (many waves adding to one word serialise at that word: measured, 200 us
// for 56 k disputed nodes), and voxel_stats_kernel sums the copies at the end
__device__ inline u64 *replica(u64 *counts, int64_t which) { return counts + (which % kVoxelStatReplicas) * kVoxelStats; }

__device__ inline int wave_sum(int n)
{
    for (int off = kWave / 2; off; off >>= 1) n += __shfl_down(n, off);
    return n;                                                             // in lane 0
}

__global__ __launch_bounds__(kWave) void voxel_stats_kernel(const u64 *__restrict__ counts, u64 *__restrict__ stats)
{
    if (threadIdx.x >= kVoxelStats) return;
    u64 sum = 0;
    for (int r = 0; r < kVoxelStatReplicas; ++r) sum += counts[r * kVoxelStats + threadIdx.x];
    stats[threadIdx.x] = sum;
}

__global__ __launch_bounds__(kBlock) void voxel_deposit_kernel(const float *__restrict__ v, int64_t n_vertices, const int32_t *__restrict__ faces,
                                                               int64_t n_triangles, int32_t G, double lo, double h, int32_t axis0, int64_t ray_slots,
                                                               int32_t *__restrict__ dep_base, u64 *counts)
{
    __shared__ unsigned block_counts[4];                                  // invalid, degenerate, deposits, wave faces of this workgroup
    if (threadIdx.x < 4) block_counts[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & (kWave - 1);
    const int ray = blockIdx.y;
    const int axis = axis0 + ray, b = (axis + 1) % 3, c = (axis + 2) % 3;
    int32_t *__restrict__ dep = dep_base + ray * ray_slots;
    const int64_t t = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    VoxFace f = {};
    int sg = 0, n_invalid = 0, n_degenerate = 0, n_deposits = 0;
    if (t < n_triangles) {                                                // no lane leaves early: the wave walks below need all 64
        const int32_t ia = faces[t * 3], ib = faces[t * 3 + 1], ic = faces[t * 3 + 2];
        bool valid = ia >= 0 && ib >= 0 && ic >= 0 && ia < n_vertices && ib < n_vertices && ic < n_vertices;
        int32_t ua[3], ub[3], uc[3];
        double ra[3], rb[3], rc[3];
        if (valid) {
            const bool oa = load_vertex(v, ia, lo, h, ua, ra), ob = load_vertex(v, ib, lo, h, ub, rb), oc = load_vertex(v, ic, lo, h, uc, rc);
            valid = oa && ob && oc;
        }
        if (!valid) {
            n_invalid = 1;
        } else {
            f.ab = pick(ua, b), f.ac = pick(ua, c), f.bb = pick(ub, b), f.bc = pick(ub, c), f.cb = pick(uc, b), f.cc = pick(uc, c);
            f.ra = pick(ra, axis), f.rb = pick(rb, axis), f.rc = pick(rc, axis);
            f.area = (long long)(f.bb - f.ab) * (f.cc - f.ac) - (long long)(f.bc - f.ac) * (f.cb - f.ab);
            if (f.area == 0) {
                n_degenerate = 1;
            } else {
                sg = f.area > 0 ? 1 : -1;
                // columns whose centre p S + S/2 lies within [min, max] of the corners, clipped to the grid
                f.b0 = max((min3(f.ab, f.bb, f.cb) + (kS / 2 - 1)) >> kVoxelSubcellBits, 0);
                f.c0 = max((min3(f.ac, f.bc, f.cc) + (kS / 2 - 1)) >> kVoxelSubcellBits, 0);
                const int32_t b1 = min((max3(f.ab, f.bb, f.cb) - kS / 2) >> kVoxelSubcellBits, G - 1);
                const int32_t c1 = min((max3(f.ac, f.bc, f.cc) - kS / 2) >> kVoxelSubcellBits, G - 1);
                f.nc = max(c1 - f.c0 + 1, 0);
                f.cols = max(b1 - f.b0 + 1, 0) * f.nc;
            }
        }
    }
    if (f.cols > 0 && f.cols <= kVoxelLaneColumns) {
        int32_t p = f.b0, pc = f.c0;
        for (int q = 0; q < kVoxelLaneColumns; ++q) {
            if (q >= f.cols) break;
            n_deposits += deposit_column(f, sg, p, pc, G, axis, dep);
            if (++pc == f.c0 + f.nc) pc = f.c0, ++p;
        }
    }
    u64 big = __ballot(f.cols > kVoxelLaneColumns);                       // wave-uniform
    const int n_wave = lane == 0 ? __popcll(big) : 0;
    while (big) {                                                         // at most 64 trips
        const int src = __ffsll(big) - 1;
        big &= big - 1;
        VoxFace g;
        g.ab = __shfl(f.ab, src), g.ac = __shfl(f.ac, src), g.bb = __shfl(f.bb, src), g.bc = __shfl(f.bc, src), g.cb = __shfl(f.cb, src), g.cc = __shfl(f.cc, src);
        g.ra = __shfl(f.ra, src), g.rb = __shfl(f.rb, src), g.rc = __shfl(f.rc, src);
        g.area = __shfl(f.area, src);
        g.b0 = __shfl(f.b0, src), g.c0 = __shfl(f.c0, src), g.nc = __shfl(f.nc, src), g.cols = __shfl(f.cols, src);
        const int gs = __shfl(sg, src);
        for (int q = lane; q < g.cols; q += kWave)                        // cols <= G^2
            n_deposits += deposit_column(g, gs, g.b0 + q / g.nc, g.c0 + q % g.nc, G, axis, dep);
    }
    const int sums[4] = {wave_sum(ray == 0 ? n_invalid : 0), wave_sum(n_degenerate), wave_sum(n_deposits), n_wave};
    if (lane == 0)
        for (int x = 0; x < 4; ++x)
            if (sums[x]) atomicAdd(&block_counts[x], unsigned(sums[x]));
    __syncthreads();
    if (threadIdx.x < 4 && block_counts[threadIdx.x]) {                   // one add per workgroup and count, spread over the copies
        const int slot = threadIdx.x == 0 ? kVoxelStatInvalid : (threadIdx.x == 1 ? kVoxelStatDegenerate + axis : (threadIdx.x == 2 ? kVoxelStatDeposits + axis : kVoxelStatWaveFaces));
        atomicAdd(replica(counts, blockIdx.x) + slot, u64(block_counts[threadIdx.x]));
    }
}

__device__ inline int rule_bit(int32_t w, int32_t rule) { return rule == kVoxelRuleNonzero ? w != 0 : (rule == kVoxelRulePositive ? w > 0 : (w & 1)); }

// Rays along i (axis 0) and j (axis 1).  dep: (slab, q, k) with q = j or i.  kOcc: out is the occupancy byte and gets the ray's rule bit at
// bit `axis` (stored when `first`, else OR-ed into the byte this lane alone owns); otherwise out is w, int32
template <bool kOcc>
__global__ __launch_bounds__(kBlock) void voxel_walk_kernel(const int32_t *__restrict__ dep, int32_t G, int32_t axis, int32_t rule, int32_t first, void *__restrict__ out,
                                                            u64 *counts)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t tid = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    const int64_t plane = int64_t(G) * G;
    const bool live = tid < plane;
    int32_t acc = 0;
    if (live) {
        const int64_t q = tid / G, k = tid % G;
        const int64_t obase = axis == 0 ? tid : q * plane + k;
        const int64_t ostride = axis == 0 ? plane : G;
        for (int s0 = 0; s0 < G; s0 += 8) {
            int32_t d[8];
            uint8_t prev[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) d[u] = s0 + u < G ? dep[tid + (s0 + u) * plane] : 0;
            if (kOcc && !first) {                                         // the byte this lane alone owns, with the same eight in flight
#pragma unroll
                for (int u = 0; u < 8; ++u) prev[u] = s0 + u < G ? static_cast<const uint8_t *>(out)[obase + (s0 + u) * ostride] : uint8_t(0);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (s0 + u >= G) continue;
                acc += d[u];
                const int64_t o = obase + (s0 + u) * ostride;
                if (kOcc) {
                    uint8_t *o8 = static_cast<uint8_t *>(out);
                    const uint8_t bit = uint8_t(rule_bit(acc, rule) << axis);
                    o8[o] = first ? bit : uint8_t(prev[u] | bit);
                } else {
                    static_cast<int32_t *>(out)[o] = acc;
                }
            }
        }
        acc += dep[tid + G * plane];                                      // slab G: what never closed
    }
    const int n = __popcll(__ballot(live && acc != 0));
    if (lane == 0 && n) atomicAdd(replica(counts, blockIdx.x) + kVoxelStatOpen + axis, u64(n));
}

// The ray along k (axis 2).  dep: rows (i, j) of G + 1 slabs.  One wave per row.  kOcc: the byte holds the bits of rays 0 and 1; the vote
// of the three replaces it, and the nodes at which they differ are counted
template <bool kOcc>
__global__ __launch_bounds__(kBlock) void voxel_row_kernel(const int32_t *__restrict__ dep, int32_t G, int32_t rule, void *__restrict__ out, u64 *counts)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t row = (int64_t(blockIdx.x) * kBlock + threadIdx.x) / kWave;
    if (row >= int64_t(G) * G) return;                                   // a whole wave at a time
    const int32_t *__restrict__ src = dep + row * (G + 1);
    int32_t carry = 0;
    int n_disputed = 0;
    for (int s0 = 0; s0 <= G; s0 += kWave) {
        const int s = s0 + lane;
        int32_t x = s <= G ? src[s] : 0;
        for (int off = 1; off < kWave; off <<= 1) {
            const int32_t y = __shfl_up(x, off);
            if (lane >= off) x += y;
        }
        x += carry;
        if (s < G) {
            const int64_t o = row * G + s;
            if (kOcc) {
                uint8_t *o8 = static_cast<uint8_t *>(out);
                const int prev = o8[o];
                const int votes = (prev & 1) + ((prev >> 1) & 1) + rule_bit(x, rule);
                o8[o] = uint8_t(votes >= 2);
                n_disputed += votes == 1 || votes == 2;
            } else {
                static_cast<int32_t *>(out)[o] = x;
            }
        } else if (s == G && x != 0) {
            atomicAdd(replica(counts, row) + kVoxelStatOpen + 2, u64(1)); // one lane per row at most
        }
        carry = __shfl(x, kWave - 1);
    }
    if (kOcc) {
        n_disputed = wave_sum(n_disputed);
        if (lane == 0 && n_disputed) atomicAdd(replica(counts, row) + kVoxelStatDisputed, u64(n_disputed));
    }
}

// workspace: the copies of the counts, then the deposits of each ray
inline u64 *counts_of(void *workspace) { return static_cast<u64 *>(workspace); }
inline int32_t *deposits_of(void *workspace) { return reinterpret_cast<int32_t *>(static_cast<char *>(workspace) + kVoxelCountBytes); }

hipError_t clear(void *workspace, int64_t slots, hipStream_t stream)
{
    return hipMemsetAsync(workspace, 0, size_t(kVoxelCountBytes) + size_t(slots) * sizeof(int32_t), stream);
}

void deposit(const float *v, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, int32_t G, double lo, double hi, int32_t axis0, int32_t rays,
             void *workspace, hipStream_t stream)
{
    if (n_triangles == 0) return;
    const double h = (hi - lo) / double(G);
    voxel_deposit_kernel<<<dim3(blocks_for(n_triangles), unsigned(rays)), kBlock, 0, stream>>>(v, n_vertices, faces, n_triangles, G, lo, h, axis0, voxel_ray_slots(G),
                                                                                                deposits_of(workspace), counts_of(workspace));
}

}  // namespace

hipError_t launch_voxel_winding(const float *v, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, int32_t grid, double lo, double hi, int32_t axis,
                                void *workspace, int32_t *w_out, int64_t *stats_out, hipStream_t stream)
{
    hipError_t e = clear(workspace, voxel_ray_slots(grid), stream);
    if (e != hipSuccess) return e;
    deposit(v, n_vertices, faces, n_triangles, grid, lo, hi, axis, 1, workspace, stream);
    const int64_t plane = int64_t(grid) * grid;
    if (axis < 2)
        voxel_walk_kernel<false><<<blocks_for(plane), kBlock, 0, stream>>>(deposits_of(workspace), grid, axis, 0, 1, w_out, counts_of(workspace));
    else
        voxel_row_kernel<false><<<blocks_for(plane * kWave), kBlock, 0, stream>>>(deposits_of(workspace), grid, 0, w_out, counts_of(workspace));
    voxel_stats_kernel<<<1, kWave, 0, stream>>>(counts_of(workspace), reinterpret_cast<u64 *>(stats_out));
    return hipGetLastError();
}

hipError_t launch_voxel_occupancy(const float *v, int64_t n_vertices, const int32_t *faces, int64_t n_triangles, int32_t grid, double lo, double hi, int32_t rule,
                                  int32_t rays, void *workspace, uint8_t *occ_out, int64_t *stats_out, hipStream_t stream)
{
    const int64_t slots = voxel_ray_slots(grid);
    hipError_t e = clear(workspace, rays * slots, stream);
    if (e != hipSuccess) return e;
    deposit(v, n_vertices, faces, n_triangles, grid, lo, hi, 0, rays, workspace, stream);
    const int64_t plane = int64_t(grid) * grid;
    int32_t *dep = deposits_of(workspace);
    voxel_walk_kernel<true><<<blocks_for(plane), kBlock, 0, stream>>>(dep, grid, 0, rule, 1, occ_out, counts_of(workspace));
    if (rays == 3) {
        voxel_walk_kernel<true><<<blocks_for(plane), kBlock, 0, stream>>>(dep + slots, grid, 1, rule, 0, occ_out, counts_of(workspace));
        voxel_row_kernel<true><<<blocks_for(plane * kWave), kBlock, 0, stream>>>(dep + 2 * slots, grid, rule, occ_out, counts_of(workspace));
    }
    voxel_stats_kernel<<<1, kWave, 0, stream>>>(counts_of(workspace), reinterpret_cast<u64 *>(stats_out));
    return hipGetLastError();
}

}  // namespace tsamd
