// Device helpers of the renderer slice: the one statement of everything more than one renderer kernel uses (raster_kernels.hip,
// interpolate_kernels.hip, term_kernels.hip).
//
// EVERY unit that includes this header must be compiled with -ffp-contract=off (tssplat_amd/_build.py: SOURCE_FLAGS;
// tests/test_build_metadata.py checks the flag): the operations of these helpers and their order are the contract -- a multiply
// and an add must round separately -- and that is what makes the kernels of different units agree to the bit.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace tsamd {

constexpr unsigned long long kNoFragment = 0xFFFFFFFFFFFFFFFFull;

// The homogeneous edge functions of a pixel centre against the clip-space triangle (v0, v1, v2): what the barycentrics of the
// resolve pass are ratios of and what rasterize_backward's quotient rule differentiates.  ONE statement of the expressions for
// every kernel that needs (u, v): the operations and their order are part of the contract (compiled without contraction), so
// the kernels agree to the bit.
struct EdgeFunctions {
    float fx, fy;                           // the pixel centre in normalised device coordinates
    float p0x, p0y, p1x, p1y, p2x, p2y;     // v_k.xy - f v_k.w
    float a0, a1;                           // u = a0 / s, v = a1 / s
    float s;                                // a0 + a1 + a2, 1 where that sum is 0
};

__device__ __forceinline__ EdgeFunctions edge_functions(const float4 v0, const float4 v1, const float4 v2, int px, int py, int height, int width)
{
    EdgeFunctions e;
    e.fx = (float(px) + 0.5f) / float(width) * 2.f - 1.f, e.fy = (float(py) + 0.5f) / float(height) * 2.f - 1.f;
    e.p0x = v0.x - e.fx * v0.w, e.p0y = v0.y - e.fy * v0.w;
    e.p1x = v1.x - e.fx * v1.w, e.p1y = v1.y - e.fy * v1.w;
    e.p2x = v2.x - e.fx * v2.w, e.p2y = v2.y - e.fy * v2.w;
    e.a0 = e.p1x * e.p2y - e.p1y * e.p2x, e.a1 = e.p2x * e.p0y - e.p2y * e.p0x;
    const float a2 = e.p0x * e.p1y - e.p0y * e.p1x;
    const float s = e.a0 + e.a1 + a2;
    e.s = s == 0.f ? 1.f : s;
    return e;
}

__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

// d (u, v) / d clip-space (x, y, w) of the three vertices, times the gradient (gu, gv): the quotient rule of u = a0 / s, v = a1 / s
// (oracle/raster_oracle.py::rasterize_backward), the clamps of the forward treated as inactive.  d[3 k ..] = (x, y, w) of vertex k.
__device__ __forceinline__ void edge_functions_backward(const EdgeFunctions &e, float gu, float gv, float d[9])
{
    const float is = 1.f / e.s;
    const float u = e.a0 * is, v = e.a1 * is;
    const float dot = gu * u + gv * v;
    const float da0 = (gu - dot) * is, da1 = (gv - dot) * is, da2 = -dot * is;
    d[0] = da1 * -e.p2y + da2 * e.p1y, d[1] = da1 * e.p2x + da2 * -e.p1x;
    d[3] = da0 * e.p2y + da2 * -e.p0y, d[4] = da0 * -e.p2x + da2 * e.p0x;
    d[6] = da0 * -e.p1y + da1 * e.p0y, d[7] = da0 * e.p1x + da1 * -e.p0x;
    d[2] = -e.fx * d[0] - e.fy * d[1];
    d[5] = -e.fx * d[3] - e.fy * d[4];
    d[8] = -e.fx * d[6] - e.fy * d[7];
}

// ---- scatter with runs ----
// The backward scatters add one value per pixel to the three vertices of the pixel's triangle.  Consecutive pixels of a row
// mostly belong to the same triangle (a 41 k-tet object at 512^2: runs of ~5), so the lanes of a run are summed inside the wave
// first -- a segmented scan over equal keys -- and only the last lane of every run issues the atomics.  A wave without any run
// (a dense scene of sub-pixel triangles) skips the scan.  EVERY lane of the wave must call these (no early return before).
struct Runs {
    int start;      // lane index of the first lane of this lane's run
    bool last;      // this lane ends its run: it holds the run's sums after run_sum()
    bool any;       // wave-uniform: some run is longer than one lane
};

__device__ __forceinline__ Runs find_runs(long long key)
{
    const int lane = int(threadIdx.x) & 63;
    const long long prev = __shfl_up(key, 1);
    const bool head = lane == 0 || key != prev;
    const unsigned long long heads = __ballot(head);
    Runs r;
    r.start = 63 - __clzll(heads & (~0ull >> (63 - lane)));
    r.last = lane == 63 || ((heads >> (lane + 1)) & 1ull) != 0ull;
    r.any = heads != ~0ull;
    return r;
}

__device__ __forceinline__ float run_sum(const Runs &r, float v)
{
    if (!r.any) return v;
    const int lane = int(threadIdx.x) & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float up = __shfl_up(v, d);
        if (lane - d >= r.start) v += up;
    }
    return v;
}

// Triangle named by a rast pixel's fourth channel (id + 1 as a float, exact up to 2^24 - 1 triangles: tsamd_rasterize
// refuses longer lists), or -1 for background / an id outside [0, n_tri) / a non-finite value.
__device__ __forceinline__ int64_t triangle_of(float w, int64_t n_tri)
{
    if (!(w >= 1.f) || !(w <= 16777216.f)) return -1;
    const int64_t t = int64_t(w) - 1;
    return t < n_tri ? t : -1;
}
// The three vertex indices of triangle t; false when one of them lies outside [0, n_vertices).
__device__ __forceinline__ bool triangle_indices(const int32_t *tri, int64_t t, int64_t n_vertices, int32_t &i0, int32_t &i1, int32_t &i2)
{
    i0 = tri[3 * t], i1 = tri[3 * t + 1], i2 = tri[3 * t + 2];
    return uint64_t(i0) < uint64_t(n_vertices) && uint64_t(i1) < uint64_t(n_vertices) && uint64_t(i2) < uint64_t(n_vertices)
           && i0 >= 0 && i1 >= 0 && i2 >= 0;
}

// Triangle named by an id of the alpha stage (triangle + 1, 0 = background) and its vertex indices; false for background, an id
// outside [1, n_tri] and a vertex index outside [0, n_vertices): nothing is read through those (as triangle_of / triangle_indices)
__device__ __forceinline__ bool triangle_of_id(int32_t id, const int32_t *tri, int64_t n_tri, int64_t n_vertices, int32_t &i0, int32_t &i1, int32_t &i2)
{
    if (id < 1 || int64_t(id) > n_tri) return false;
    return triangle_indices(tri, int64_t(id) - 1, n_vertices, i0, i1, i2);
}

// What every id-driven term starts from at a covered pixel (px, py) of a view with clip-space vertices pv: the clamped barycentrics
// of the resolve pass, w = (1 - u) - v as interpolate_kernel forms it, and the three rows of a 3-channel vertex attribute,
// a[3 k + c] = channel c of vertex i_k.  (ONE statement of these operations for every term and both directions.)
__device__ __forceinline__ EdgeFunctions weights_and_gather(const float4 *pv, const float *attr, int32_t i0, int32_t i1, int32_t i2, int px, int py, int height,
                                                            int width, float &u, float &v, float &w, float a[9])
{
    const EdgeFunctions e = edge_functions(pv[i0], pv[i1], pv[i2], px, py, height, width);
    u = clamp01(e.a0 / e.s), v = clamp01(e.a1 / e.s);
    w = 1.f - u - v;
    const float *a0 = attr + 3 * int64_t(i0), *a1 = attr + 3 * int64_t(i1), *a2 = attr + 3 * int64_t(i2);
#pragma unroll
    for (int k = 0; k < 3; ++k) a[k] = a0[k], a[3 + k] = a1[k], a[6 + k] = a2[k];
    return e;
}

// view, row and column of pixel gid; b0 = the view of the wave's first pixel (a wave of `span` pixels crosses at most one view
// boundary when hw >= span), as in the resolve pass
__device__ __forceinline__ void locate_pixel(int64_t gid, int64_t hw, int width, bool one_boundary, int64_t b0, int64_t &b, int &px, int &py)
{
    uint32_t pix;
    if (one_boundary) {
        const int64_t off = gid - b0 * hw;
        b = off >= hw ? b0 + 1 : b0;
        pix = uint32_t(off >= hw ? off - hw : off);
    } else {
        b = gid / hw;
        pix = uint32_t(gid - b * hw);
    }
    py = int(pix / uint32_t(width));   // (pix < 2^26: height, width <= 8192)
    px = int(pix - uint32_t(py) * uint32_t(width));
}

// The K consecutive 64-pixel chunks a wave of the resolve pass, the cover pass and the forward term kernels holds, gid0 (wave-uniform)
// its first pixel: pixel k of a lane is the lane-th pixel of chunk k, so every load of a wave is one contiguous run of 64 elements.
// view / row / column without a per-lane 64-bit division: the view of the wave's first pixel on the scalar unit (a wave crosses at
// most one view boundary unless the image has fewer than 64 K pixels).
template <int K>
struct WavePixels {
    int64_t gid0, gid[K], b[K];   // flat pixel index; view
    int px[K], py[K];             // column, row
    bool have[K];                 // gid < total
};

template <int K>
__device__ __forceinline__ WavePixels<K> wave_pixels(int64_t gid0, int lane, int64_t total, int64_t hw, int width)
{
    WavePixels<K> p;
    p.gid0 = gid0;
    const bool one_boundary = hw >= 64 * K;
    const int64_t b0 = one_boundary ? gid0 / hw : 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        p.gid[k] = gid0 + 64 * k + lane;
        p.have[k] = p.gid[k] < total;
        locate_pixel(p.gid[k], hw, width, one_boundary, b0, p.b[k], p.px[k], p.py[k]);
    }
    return p;
}

// The depth keys of a wave's pixels and of the neighbours the pair masks compare them with: the pixel above (key_up) and, for
// lane 63 of the last chunk, the pixel to the right (key_right: the right neighbour of any other chunk's last pixel is the next
// chunk's first, a lane of this wave).  neighbours = false: only `key` is loaded.  ALL loads are issued here, together, before
// any use: the kernels are bound by the latency of their key loads (a second round trip behind the first costs as much again).
// want_right needs no `gid + 1 < total`: px + 1 < width puts pixel gid + 1 into the same row of the same view.
template <int K>
struct WaveKeys {
    unsigned long long key[K], key_up[K], key_right;   // kNoFragment where not loaded
    bool want_up[K], want_right;
};

template <int K>
__device__ __forceinline__ WaveKeys<K> load_keys(const unsigned long long *keys, const WavePixels<K> &p, int lane, int height, int width, bool neighbours)
{
    WaveKeys<K> q;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        q.want_up[k] = neighbours && p.have[k] && p.py[k] + 1 < height;
        q.key[k] = p.have[k] ? keys[p.gid[k]] : kNoFragment;
        q.key_up[k] = q.want_up[k] ? keys[p.gid[k] + width] : kNoFragment;
    }
    q.want_right = neighbours && p.have[K - 1] && p.px[K - 1] + 1 < width && lane == 63;
    q.key_right = kNoFragment;
    if (q.want_right) q.key_right = keys[p.gid0 + 64 * K];   // (= gid[K - 1] + 1 of lane 63, spelled wave-uniform: a scalar load)
    return q;
}

// The pair masks of a wave's pixels, two 64-bit words per 64 pixels at masks[2 (gid >> 6)]: bit l of the first word says that
// pixel l of the chunk and its right neighbour are of different classes, bit l of the second the same for the upper neighbour;
// no bit for a pair that leaves the image.  cls(key) is the pixel's class as a uint32_t.  The right neighbour inside the wave
// comes from a shift of the classes by one lane (every lane takes part: lane 62 reads lane 63).
template <int K, class Class>
__device__ __forceinline__ void store_pair_masks(unsigned long long *masks, const WavePixels<K> &p, const WaveKeys<K> &q, int lane, int height, int width,
                                                 Class cls)
{
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint32_t own = cls(q.key[k]);
        const uint32_t next = uint32_t(__shfl_down(int(own), 1));
        uint32_t beyond = own;                                      // lane 63's right neighbour
        if (k + 1 < K)
            beyond = uint32_t(__builtin_amdgcn_readfirstlane(int(cls(q.key[k + 1 < K ? k + 1 : k]))));
        else if (q.want_right)
            beyond = cls(q.key_right);
        const uint32_t right = lane == 63 ? beyond : next;
        const uint32_t up = q.want_up[k] ? cls(q.key_up[k]) : own;
        const bool c0 = p.have[k] && p.px[k] + 1 < width && right != own;
        const bool c1 = p.have[k] && p.py[k] + 1 < height && up != own;
        const unsigned long long m0 = __ballot(c0), m1 = __ballot(c1);
        if (lane == 0 && p.have[k]) {
            masks[2 * (p.gid[k] >> 6)] = m0;
            masks[2 * (p.gid[k] >> 6) + 1] = m1;
        }
    }
}

}  // namespace tsamd
