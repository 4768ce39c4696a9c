// gfx950 kernels of the tet-sphere merge: tet mesh -> union field on the voxel grid -> marching tetrahedra -> one closed surface.
//   union_field_kernel     one wave per (tet, slab of 16 node planes), lanes over the nodes of the tet's dilated box in the slab,
//                          k fastest; f = max over tets of (min over the four faces of the distance to the face plane) through an
//                          integer atomicMax on the order-preserving image of the float32, tried only where a plain read shows
//                          that it would raise the value
//   union_decode_kernel    key image -> float32 in place, -inf where no tet reached the node
//   surface_count_kernel   one lane per node: the mask of its owned edges that change sign, the triangle count of its cube, and
//                          whether a border node is inside
//   surface_emit_kernel    one lane per node: its vertices at offset + rank, its cube's triangles at offset, winding from the
//                          permutation parity
// Semantics: tests/union_oracle.py.  float64 throughout on float32 inputs, every operation rounded on its own
// (-ffp-contract=off, _build.py; IEEE division and square root), minimum and maximum by comparisons, the maximum on integers:
// the results are bitwise repeatable and equal the oracle's.  No float atomics, no tables.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "merge.h"

namespace tsamd {

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kSlab = 16;            // node planes (index i) per wave of the field kernel: a tet spanning the grid is cut into G / 16 pieces

// Order-preserving image of a float32 that is not a NaN: a < b  <=>  key(a) < key(b); every key is > 0, so 0 means "nothing yet".
__device__ inline uint32_t key_of(float v)
{
    uint32_t u = __float_as_uint(v);
    if ((u << 1) == 0) u = 0;                                 // -0.0 is stored as +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ inline float value_of(uint32_t key)
{
    if (key == 0) return __uint_as_float(0xFF800000u);        // -inf: no tet covers the node
    return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}

__device__ inline bool finite_bits(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

// [ceil((mn - lo) / h - 0.5) - 1, floor((mx - lo) / h - 0.5) + 1] clipped to [0, G - 1]; false when empty.  All inputs are finite.
__device__ inline bool axis_box(double mn, double mx, double lo, double h, int32_t grid, int32_t &first, int32_t &last)
{
    const double a = fmax(ceil((mn - lo) / h - 0.5) - 1.0, 0.0);
    const double b = fmin(floor((mx - lo) / h - 0.5) + 1.0, double(grid - 1));
    if (!(a <= b)) return false;
    first = int32_t(a);
    last = int32_t(b);
    return true;
}

struct Plane {
    double nx, ny, nz;
};

// unit normal of the face (q, r, s): (r - q) x (s - q), normalised by one square root and three divisions
__device__ inline Plane face_plane(const double *q, const double *r, const double *s)
{
    const double ux = r[0] - q[0], uy = r[1] - q[1], uz = r[2] - q[2];
    const double wx = s[0] - q[0], wy = s[1] - q[1], wz = s[2] - q[2];
    const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
    const double len = __dsqrt_rn((nx * nx + ny * ny) + nz * nz);
    return {nx / len, ny / len, nz / len};
}

__global__ __launch_bounds__(kBlock) void union_field_kernel(const float *__restrict__ tet_v, int64_t n_vertices, const int32_t *__restrict__ elem,
                                                             int64_t n_tets, int32_t grid, double lo, double h, uint32_t *keys)
{
    const int64_t t = int64_t(blockIdx.x) * kWaves + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (t >= n_tets) return;                                  // wave-uniform, like every return below
    int32_t id[4];
    for (int c = 0; c < 4; ++c) {
        id[c] = elem[t * 4 + c];
        if (id[c] < 0 || id[c] >= n_vertices) return;         // nothing is read through a bad index
    }
    // the first axis alone decides whether this wave's slab meets the tet's box: most waves of a tall grid leave here
    double p[4][3];
    for (int c = 0; c < 4; ++c) {
        const float x = tet_v[int64_t(id[c]) * 3];
        if (!finite_bits(x)) return;
        p[c][0] = double(x);
    }
    int32_t first[3], last[3];
    if (!axis_box(fmin(fmin(p[0][0], p[1][0]), fmin(p[2][0], p[3][0])), fmax(fmax(p[0][0], p[1][0]), fmax(p[2][0], p[3][0])), lo, h, grid, first[0], last[0]))
        return;
    const int32_t i0 = max(first[0], int32_t(blockIdx.y) * kSlab), i1 = min(last[0], int32_t(blockIdx.y) * kSlab + kSlab - 1);
    if (i0 > i1) return;
    for (int c = 0; c < 4; ++c)
        for (int ax = 1; ax < 3; ++ax) {
            const float x = tet_v[int64_t(id[c]) * 3 + ax];
            if (!finite_bits(x)) return;
            p[c][ax] = double(x);
        }
    for (int ax = 1; ax < 3; ++ax) {
        const double mn = fmin(fmin(p[0][ax], p[1][ax]), fmin(p[2][ax], p[3][ax]));
        const double mx = fmax(fmax(p[0][ax], p[1][ax]), fmax(p[2][ax], p[3][ax]));
        if (!axis_box(mn, mx, lo, h, grid, first[ax], last[ax])) return;
    }
    {   // signed volume (b - a) . ((c - a) x (d - a)) > 0
        const double e1x = p[1][0] - p[0][0], e1y = p[1][1] - p[0][1], e1z = p[1][2] - p[0][2];
        const double e2x = p[2][0] - p[0][0], e2y = p[2][1] - p[0][1], e2z = p[2][2] - p[0][2];
        const double e3x = p[3][0] - p[0][0], e3y = p[3][1] - p[0][1], e3z = p[3][2] - p[0][2];
        const double cx = e2y * e3z - e2z * e3y, cy = e2z * e3x - e2x * e3z, cz = e2x * e3y - e2y * e3x;
        const double vol = (e1x * cx + e1y * cy) + e1z * cz;
        if (!(vol > 0.0)) return;
    }
    // faces opposite a, b, c, d: (b, d, c), (a, c, d), (a, d, b), (a, b, c); their normals point at the opposite corner
    const Plane f0 = face_plane(p[1], p[3], p[2]), f1 = face_plane(p[0], p[2], p[3]), f2 = face_plane(p[0], p[3], p[1]), f3 = face_plane(p[0], p[1], p[2]);
    const int32_t nj = last[1] - first[1] + 1, nk = last[2] - first[2] + 1;
    const int32_t count = (i1 - i0 + 1) * nj * nk;            // <= 16 x 512 x 512
    for (int32_t e = lane; e < count; e += 64) {
        const int32_t r = e / nk, k = first[2] + (e - r * nk), ii = r / nj, j = first[1] + (r - ii * nj), i = i0 + ii;
        const double px = lo + (double(i) + 0.5) * h, py = lo + (double(j) + 0.5) * h, pz = lo + (double(k) + 0.5) * h;
        const double ax = px - p[0][0], ay = py - p[0][1], az = pz - p[0][2];
        const double d0 = (f0.nx * (px - p[1][0]) + f0.ny * (py - p[1][1])) + f0.nz * (pz - p[1][2]);
        const double d1 = (f1.nx * ax + f1.ny * ay) + f1.nz * az;
        const double d2 = (f2.nx * ax + f2.ny * ay) + f2.nz * az;
        const double d3 = (f3.nx * ax + f3.ny * ay) + f3.nz * az;
        double m = d0;
        if (d1 < m) m = d1;
        if (d2 < m) m = d2;
        if (d3 < m) m = d3;
        if (!(m == m)) continue;                              // a NaN never replaces a number
        const uint32_t key = key_of(float(m));
        uint32_t *dst = keys + ((int64_t(i) * grid + j) * grid + k);
        // the value only grows, so a stale read can only cause an atomic that changes nothing, never skip one that would
        if (__atomic_load_n(dst, __ATOMIC_RELAXED) < key) atomicMax(dst, key);
    }
}

__global__ __launch_bounds__(kBlock) void union_decode_kernel(uint32_t *keys, int32_t n)
{
    const int32_t v = int32_t(blockIdx.x) * kBlock + threadIdx.x;
    if (v < n) reinterpret_cast<float *>(keys)[v] = value_of(keys[v]);
}

// ---- marching tetrahedra on the six Kuhn tets of every cube ----
// Corner m (mask 4 di + 2 dj + dk) of the cube at node o is node o + (di, dj, dk).  Tet p in 0 .. 5 belongs to the p-th
// permutation in lexicographic order and has the corner chain 0, bit(perm[0]), bit(perm[0]) | bit(perm[1]), 7.
__device__ inline void tet_chain(int p, int mask[4], bool &even)
{
    const int a0 = p >> 1;
    const int lower = a0 == 0 ? 1 : 0, upper = a0 == 2 ? 1 : 2;      // the two other axes, in order
    const int a1 = (p & 1) ? upper : lower;
    mask[0] = 0;
    mask[1] = 4 >> a0;
    mask[2] = mask[1] | (4 >> a1);
    mask[3] = 7;
    even = ((p & 1) == 0) != (a0 == 1);                       // (0,1,2) + (0,2,1) - (1,0,2) - (1,2,0) + (2,0,1) + (2,1,0) -
}

// bit m of `valid`: corner m lies in the grid; bit m of the result: it does and field > level there (a NaN is outside)
__device__ inline uint32_t corner_bits(const float *__restrict__ field, int32_t grid, int32_t i, int32_t j, int32_t k, float level, uint32_t &valid)
{
    uint32_t bits = 0;
    valid = 0;
    for (int m = 0; m < 8; ++m) {
        const int32_t ci = i + ((m >> 2) & 1), cj = j + ((m >> 1) & 1), ck = k + (m & 1);
        if (ci < grid && cj < grid && ck < grid) {
            valid |= 1u << m;
            if (field[(int64_t(ci) * grid + cj) * grid + ck] > level) bits |= 1u << m;
        }
    }
    return bits;
}

__global__ __launch_bounds__(kBlock) void surface_count_kernel(const float *__restrict__ field, int32_t grid, float level, uint8_t *__restrict__ vmask,
                                                               uint8_t *__restrict__ vcount, uint8_t *__restrict__ tcount, int32_t *open)
{
    const int32_t n = grid * grid * grid;
    const int32_t v = int32_t(blockIdx.x) * kBlock + threadIdx.x;
    bool border_inside = false;
    if (v < n) {
        const int32_t i = v / (grid * grid), r = v - i * grid * grid, j = r / grid, k = r - j * grid;
        uint32_t valid;
        const uint32_t bits = corner_bits(field, grid, i, j, k, level, valid);
        const uint32_t self = bits & 1u;
        uint32_t vm = 0;
        for (int m = 1; m < 8; ++m)
            if (((valid >> m) & 1u) && ((bits >> m) & 1u) != self) vm |= 1u << (m - 1);
        int tc = 0;
        if (valid == 0xFFu) {
            for (int p = 0; p < 6; ++p) {
                int mask[4];
                bool even;
                tet_chain(p, mask, even);
                const int nin = int((bits >> mask[0]) & 1u) + int((bits >> mask[1]) & 1u) + int((bits >> mask[2]) & 1u) + int((bits >> mask[3]) & 1u);
                tc += nin == 2 ? 2 : ((nin == 1 || nin == 3) ? 1 : 0);
            }
        }
        vmask[v] = uint8_t(vm);
        vcount[v] = uint8_t(__popc(vm));
        tcount[v] = uint8_t(tc);
        border_inside = self && (i == 0 || j == 0 || k == 0 || i == grid - 1 || j == grid - 1 || k == grid - 1);
    }
    if (__any(border_inside) && (threadIdx.x & 63) == 0) atomicOr(open, 1);
}

__global__ __launch_bounds__(kBlock) void surface_emit_kernel(const float *__restrict__ field, int32_t grid, double lo, double h, float level,
                                                              const uint8_t *__restrict__ vmask, const int32_t *__restrict__ voffset,
                                                              const int32_t *__restrict__ toffset, int64_t n_vertices, int64_t n_triangles,
                                                              float *__restrict__ v_out, int32_t *__restrict__ faces_out)
{
    const int32_t n = grid * grid * grid;
    const int32_t v = int32_t(blockIdx.x) * kBlock + threadIdx.x;
    if (v >= n) return;
    const int32_t i = v / (grid * grid), r = v - i * grid * grid, j = r / grid, k = r - j * grid;
    uint32_t valid;
    const uint32_t bits = corner_bits(field, grid, i, j, k, level, valid);
    const uint32_t vm = uint32_t(vmask[v]) & (valid >> 1);     // (an edge that leaves the grid is never followed, whatever the mask holds)
    // vertices: one per set bit of vm, at voffset + rank; a is the inside end of the edge
    if (vm != 0) {
        const double lv = double(level);
        const double own[3] = {lo + (double(i) + 0.5) * h, lo + (double(j) + 0.5) * h, lo + (double(k) + 0.5) * h};
        const double f_own = double(field[v]);
        const bool own_in = bits & 1u;
        int64_t at = voffset[v];
        for (int m = 1; m < 8; ++m) {
            if (!((vm >> (m - 1)) & 1u)) continue;
            const int32_t d[3] = {(m >> 2) & 1, (m >> 1) & 1, m & 1};
            const double other[3] = {lo + (double(i + d[0]) + 0.5) * h, lo + (double(j + d[1]) + 0.5) * h, lo + (double(k + d[2]) + 0.5) * h};
            const double f_other = double(field[(int64_t(i + d[0]) * grid + (j + d[1])) * grid + (k + d[2])]);
            const double fa = own_in ? f_own : f_other, fb = own_in ? f_other : f_own;
            double t = (fa - lv) / (fa - fb);
            if (!(t >= 0.0 && t <= 1.0)) t = 0.0;               // only with a non-finite value at an end
            if (at >= 0 && at < n_vertices) {
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    const double pa = own_in ? own[ax] : other[ax], pb = own_in ? other[ax] : own[ax];
                    v_out[at * 3 + ax] = float(pa + t * (pb - pa));
                }
            }
            ++at;
        }
    }
    if (valid != 0xFFu) return;
    // triangles of the cube at this node, tet by tet.  Chain positions are kept in 2-bit fields of plain integers, not in arrays.
    int64_t slot = toffset[v];
    for (int p = 0; p < 6; ++p) {
        int mask[4];
        bool even;
        tet_chain(p, mask, even);
        const uint32_t chain = uint32_t(mask[1]) << 3 | uint32_t(mask[2]) << 6 | 7u << 9;                // corner mask of chain position c: bits 3 c ..
        uint32_t ins = 0, outs = 0;                                                                  // chain positions inside / outside, in order
        int nf = 0, nr = 0;
#pragma unroll
        for (uint32_t c = 0; c < 4; ++c) {
            if ((bits >> ((chain >> (3 * c)) & 7u)) & 1u) ins |= c << (2 * nf++);
            else outs |= c << (2 * nr++);
        }
        if (nf == 0 || nf == 4) continue;
        const bool flip = nf == 3;                              // one corner outside: the first case with the roles exchanged, reversed
        const uint32_t arr = flip ? (outs | ins << (2 * nr)) : (ins | outs << (2 * nf));
        const int a = arr & 3u, b = (arr >> 2) & 3u;
        int c = (arr >> 4) & 3u, d = (arr >> 6) & 3u;
        const int inv = (a > b) + (a > c) + (a > d) + (b > c) + (b > d) + (c > d);
        if (((inv & 1) == 0) != even) {                         // negative arrangement: exchange its last two corners
            const int s = c;
            c = d;
            d = s;
        }
        // the vertex on the edge between chain positions x and y: owned by the node of the lower corner
        auto vertex = [&](int x, int y) -> int32_t {
            const uint32_t mx = (chain >> (3 * (x < y ? x : y))) & 7u, my = (chain >> (3 * (x < y ? y : x))) & 7u;
            const int32_t owner = v + int32_t((((mx >> 2) & 1u) * grid + ((mx >> 1) & 1u)) * grid + (mx & 1u));
            return voffset[owner] + __popc(uint32_t(vmask[owner]) & ((1u << ((mx ^ my) - 1u)) - 1u));
        };
        int32_t t0, t1, t2;
        if (nf == 2) {                                          // a, b inside: (ac, ad, bd) and (ac, bd, bc)
            t0 = vertex(a, c), t1 = vertex(a, d), t2 = vertex(b, d);
            if (slot >= 0 && slot < n_triangles) {
                faces_out[slot * 3 + 0] = t0;
                faces_out[slot * 3 + 1] = t1;
                faces_out[slot * 3 + 2] = t2;
            }
            ++slot;
            t1 = t2;
            t2 = vertex(b, c);
        } else {                                                // a alone on its side: (ab, ac, ad), reversed when a is the outside one
            t0 = vertex(a, b), t1 = vertex(a, c), t2 = vertex(a, d);
        }
        if (slot >= 0 && slot < n_triangles) {
            faces_out[slot * 3 + 0] = t0;
            faces_out[slot * 3 + 1] = flip ? t2 : t1;
            faces_out[slot * 3 + 2] = flip ? t1 : t2;
        }
        ++slot;
    }
}

unsigned blocks_for(int64_t n, int per_block) { return unsigned((n + per_block - 1) / per_block); }

}  // namespace

hipError_t launch_union_field(const float *tet_v, int64_t n_vertices, const int32_t *elem, int64_t n_tets, int32_t grid, double lo, double step,
                              float *field, hipStream_t stream)
{
    const int64_t n = int64_t(grid) * grid * grid;
    uint32_t *keys = reinterpret_cast<uint32_t *>(field);
    hipError_t e = hipMemsetAsync(keys, 0, size_t(n) * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    if (n_tets > 0)
        union_field_kernel<<<dim3(blocks_for(n_tets, kWaves), blocks_for(grid, kSlab)), kBlock, 0, stream>>>(tet_v, n_vertices, elem, n_tets, grid, lo, step, keys);
    union_decode_kernel<<<blocks_for(n, kBlock), kBlock, 0, stream>>>(keys, int32_t(n));
    return hipGetLastError();
}

hipError_t launch_surface_count(const float *field, int32_t grid, float level, uint8_t *vmask, uint8_t *vcount, uint8_t *tcount, int32_t *open,
                                hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(open, 0, sizeof(int32_t), stream);
    if (e != hipSuccess) return e;
    const int64_t n = int64_t(grid) * grid * grid;
    surface_count_kernel<<<blocks_for(n, kBlock), kBlock, 0, stream>>>(field, grid, level, vmask, vcount, tcount, open);
    return hipGetLastError();
}

hipError_t launch_surface_emit(const float *field, int32_t grid, double lo, double step, float level, const uint8_t *vmask, const int32_t *voffset,
                               const int32_t *toffset, int64_t n_vertices, int64_t n_triangles, float *v_out, int32_t *faces_out, hipStream_t stream)
{
    const int64_t n = int64_t(grid) * grid * grid;
    surface_emit_kernel<<<blocks_for(n, kBlock), kBlock, 0, stream>>>(field, grid, lo, step, level, vmask, voffset, toffset, n_vertices, n_triangles, v_out,
                                                                      faces_out);
    return hipGetLastError();
}

}  // namespace tsamd
