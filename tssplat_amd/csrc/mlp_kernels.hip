// gfx950 kernels of the fully fused MLP (mlp.h; semantics: tests/mlp_oracle.py).
//
//   mlp_forward_kernel    persistent workgroups of four waves; each wave takes 16 rows of a 64-row block and runs the whole
//                         network on chip.  A layer computes H^T = W . X^T with v_mfma_f32_16x16x32_f16: the batch row is the
//                         accumulator's column (lane & 15), the neuron its row (4 (lane >> 4) + reg), so the accumulator
//                         tiles of one layer, converted to fp16 pairwise, ARE the B operand of the next (no LDS round trip).
//   mlp_backward_kernel   recomputes the forward of its rows in registers (no stored activations), carries delta down the
//                         network in the same layout (delta_{m-1}^T = W_m^T . delta_m^T), writes dx, and accumulates dW of
//                         one group of matrices in fp32 MFMA accumulators over all its rows.  dW sums over the ROW index, which
//                         lives on the lanes: delta and the layer input go through LDS as [neuron][row] images, each wave
//                         owning a fixed set of 16 x 16 dW tiles.  Each workgroup writes one partial per parameter to the
//                         workspace; a network whose dW does not fit one pass loops the same kernel over groups of matrices.
//   mlp_reduce_kernel     sums the partials in workgroup order and divides by the loss scale: no float atomics anywhere, so
//                         y, dx and dW are bitwise repeatable for a given number of rows.
//
// Weights live in LDS as fp16 A-operand fragment images (one 16-byte ds_read per lane per MFMA, conflict-free), built from
// the fp32 params by the workgroup itself: once per workgroup when the network fits kMlpResidentBytes, else one matrix at a
// time per row block.
//
// MFMA operand map used throughout (the A and B maps share the k order, so any bijection of k works): within a k-step of 32,
// lane l (c = l & 15, q = l >> 4) holds element j of A row c / B column c at k = kmap(j, q) = 16 (j >> 2) + 4 q + (j & 3).
// That is exactly where accumulator tiles 2s (j < 4) and 2s + 1 (j >= 4) keep neuron 32 s + k of the lane's row: C/D of
// 16x16x32 holds column l & 15, row 4 (l >> 4) + reg.
#include <hip/hip_runtime.h>

#include "mlp.h"

namespace tsamd {
namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float float4v __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kActNone = 0, kActRelu = 1, kActSigmoid = 2;
constexpr int kFwdMaxBlocks = 2048;

struct MlpArgs {
    MlpShape s;
    int32_t resident;                       // 1: every image below staged once per workgroup
    int32_t fwd_off[kMlpMaxHidden + 1];     // LDS offset (halfs) of matrix m's fragment image (resident)
    int32_t tr_off[kMlpMaxHidden + 1];      // ... of its transpose's (backward, resident)
    int32_t img_off;                        // LDS offset (halfs) of the backward's delta image; the input image follows
    int32_t img_a_off;
    int32_t lo, hi;                         // matrices whose dW this pass accumulates (lo > hi: none)
    int32_t down_to;                        // lowest matrix whose delta this pass needs
    int32_t want_dx;
    int32_t tile_off[kMlpMaxHidden + 2];    // first dW tile of matrix m within the pass
    int32_t n_tiles;
    int32_t vec;                            // x rows are 16-byte aligned (n_in % 4 == 0): float4 loads
};

__device__ __forceinline__ int kmap(int j, int q) { return 16 * (j >> 2) + 4 * q + (j & 3); }

__device__ __forceinline__ float4v mfma(const half8 &a, const half8 &b, const float4v &c)
{
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ half8 frag(const _Float16 *img, int rt, int nks, int ks, int lane)
{
    return *reinterpret_cast<const half8 *>(img + ((rt * nks + ks) * 64 + lane) * 8);
}

// Fragment image of the A operand `W` ([R, K] row-major) or of W^T: fragment (rt, ks) holds, for lane (i, q), element j =
// A[16 rt + i][32 ks + kmap(j, q)] (0 past A's columns).  All threads of the workgroup take part.
__device__ void stage_image(_Float16 *lds, const float *__restrict__ w, int R, int K, bool tr)
{
    const int rows = tr ? K : R, cols = tr ? R : K;
    const int nks = (cols + 31) / 32;
    const int n = (rows / 16) * nks * 64;
    for (int f = threadIdx.x; f < n; f += kThreads) {
        const int lane = f & 63, fr = f >> 6;
        const int rt = fr / nks, ks = fr - rt * nks;
        const int i = 16 * rt + (lane & 15), q = lane >> 4;
        half8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = 32 * ks + kmap(j, q);
            v[j] = static_cast<_Float16>(c < cols ? (tr ? w[int64_t(c) * K + i] : w[int64_t(i) * K + c]) : 0.0f);
        }
        *reinterpret_cast<half8 *>(lds + int64_t(f) * 8) = v;
    }
}

// B operand of matrix 0, k-step ks: x[row][32 ks + kmap(j, q)], 1.0 in the padded columns [n_in, in_w), 0 past them and on
// rows >= n.
__device__ __forceinline__ half8 load_x(const float *__restrict__ x, int64_t row, int64_t n, const MlpShape &s, int vec, int ks, int q)
{
    half8 v;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int c = 32 * ks + 16 * h + 4 * q;
        float t[4];
        if (vec && row < n && c < s.n_in) {
            const float4 f = *reinterpret_cast<const float4 *>(x + row * s.n_in + c);
            t[0] = f.x, t[1] = f.y, t[2] = f.z, t[3] = f.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                t[e] = row >= n ? 0.0f : (c + e < s.n_in ? x[row * s.n_in + c + e] : (c + e < s.in_w ? 1.0f : 0.0f));
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * h + e] = static_cast<_Float16>(t[e]);
    }
    return v;
}

// Accumulator tiles -> B operand of the next product: k-step s takes tiles 2s (elements 0..3) and 2s + 1 (4..7).
template <int NT, int KS>
__device__ __forceinline__ void pack(const float4v (&acc)[NT], half8 (&h)[KS], int act)
{
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int t = 2 * s + (j >> 2);
            float v = t < NT ? acc[t < NT ? t : 0][j & 3] : 0.0f;
            if (act == kActRelu) v = fmaxf(v, 0.0f);
            h[s][j] = static_cast<_Float16>(v);
        }
}

// The backward's stack of hidden activations, compile-time indexed only (a register array indexed by a run-time layer would
// live in scratch): push shifts everything one slot deeper, pop takes slot 0 and shifts back.
template <int KS>
__device__ __forceinline__ void push(half8 (&hs)[kMlpMaxHidden][KS], const half8 (&v)[KS])
{
#pragma unroll
    for (int i = kMlpMaxHidden - 1; i > 0; --i)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) hs[i][ks] = hs[i - 1][ks];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) hs[0][ks] = v[ks];
}

template <int KS>
__device__ __forceinline__ void pop(half8 (&hs)[kMlpMaxHidden][KS], half8 (&v)[KS])
{
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) v[ks] = hs[0][ks];
#pragma unroll
    for (int i = 0; i < kMlpMaxHidden - 1; ++i)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) hs[i][ks] = hs[i + 1][ks];
}

// e^x = 2^n 2^r with n = rint(x log2(e)) and r = x log2(e) - n from explicit fmas, log2(e) split in two floats: |r| <= 1/2
// carries 0.2 ulp of error into the result and exp2f adds its own 1 ulp.  Not expf: the compiler expands it as
// exp2((ph - rint(ph)) + pl) with ph + pl = x log2(e), and under -ffp-contract=fast (this file's mode, which no pragma
// overrides in the backend) it fuses the difference with the product ph into fma(x, log2(e), -rint(ph)).  That counts the
// rounding error of ph twice: ln 2 ulp(ph) / 2 relative in e^x, 7 ulp measured at x = 28, 22 ulp by the same count at x = 88.
__device__ __forceinline__ float exp_by_fma(float x)
{
    constexpr float kLog2eHi = 0x1.715476p+0f, kLog2eLo = 0x1.4ae0c0p-26f;
    const float n = rintf(x * kLog2eHi);
    const float r = fmaf(x, kLog2eLo, fmaf(x, kLog2eHi, -n));
    const float e = ldexpf(exp2f(r), static_cast<int>(n));
    return x < -104.0f ? 0.0f : (x > 89.0f ? __builtin_inff() : e);      // past the float range r is no longer small
}

__device__ __forceinline__ float sigmoid(float v) { return 1.0f / (1.0f + exp_by_fma(-v)); }

template <int W>
__global__ __launch_bounds__(kThreads) void mlp_forward_kernel(const float *__restrict__ x, int64_t n, const float *__restrict__ params,
                                                               MlpArgs a, float *__restrict__ y)
{
    extern __shared__ __align__(16) _Float16 lds[];
    constexpr int NT = W / 16, KS = (W + 31) / 32;
    const MlpShape &s = a.s;
    const int L = s.n_hidden;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4;
    const int ks0 = (s.in_w + 31) / 32;
    if (a.resident) {
        for (int m = 0; m <= L; ++m) stage_image(lds + a.fwd_off[m], params + s.off[m], s.rows[m], s.cols[m], false);
        __syncthreads();
    }
    auto image = [&](int m) -> const _Float16 * {
        if (a.resident) return lds + a.fwd_off[m];
        __syncthreads();
        stage_image(lds, params + s.off[m], s.rows[m], s.cols[m], false);
        __syncthreads();
        return lds;
    };
    const int64_t nblk = (n + kMlpRowsPerBlock - 1) / kMlpRowsPerBlock;
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {          // uniform over the workgroup
        const int64_t row = blk * kMlpRowsPerBlock + wave * 16 + (lane & 15);
        half8 h[KS];
        {
            const _Float16 *img = image(0);
            float4v acc[NT] = {};
            for (int ks = 0; ks < ks0; ++ks) {
                const half8 b = load_x(x, row, n, s, a.vec, ks, q);
#pragma unroll
                for (int rt = 0; rt < NT; ++rt) acc[rt] = mfma(frag(img, rt, ks0, ks, lane), b, acc[rt]);
            }
            pack(acc, h, s.act);
        }
        for (int m = 1; m < L; ++m) {
            const _Float16 *img = image(m);
            float4v acc[NT] = {};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                for (int rt = 0; rt < NT; ++rt) acc[rt] = mfma(frag(img, rt, KS, ks, lane), h[ks], acc[rt]);
            pack(acc, h, s.act);
        }
        const _Float16 *img = image(L);
        for (int rt = 0; rt < s.out_w / 16; ++rt) {
            float4v acc = {};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) acc = mfma(frag(img, rt, KS, ks, lane), h[ks], acc);
            if (row < n) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int c = 16 * rt + 4 * q + r;
                    if (c < s.n_out) y[row * s.n_out + c] = s.out_act == kActSigmoid ? sigmoid(acc[r]) : acc[r];
                }
            }
        }
    }
}

template <int W, int SLOTS>
__global__ __launch_bounds__(kThreads) void mlp_backward_kernel(const float *__restrict__ x, int64_t n, const float *__restrict__ params,
                                                                MlpArgs a, const float *__restrict__ dy, float *__restrict__ grad_x,
                                                                float *__restrict__ ws)
{
    extern __shared__ __align__(16) _Float16 lds[];
    constexpr int NT = W / 16, KS = (W + 31) / 32;
    constexpr int KD = KS > 2 ? KS : 2;                 // k-steps of delta: the hidden width, or out_w <= 64
    const MlpShape &s = a.s;
    const int L = s.n_hidden;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, col = wave * 16 + (lane & 15);
    const int ks0 = (s.in_w + 31) / 32;
    const int nto = s.out_w / 16;
    _Float16 *img_d = lds + a.img_off, *img_a = lds + a.img_a_off;
    if (a.resident) {
        for (int m = 0; m <= L; ++m) {
            stage_image(lds + a.fwd_off[m], params + s.off[m], s.rows[m], s.cols[m], false);
            if (a.tr_off[m] >= 0) stage_image(lds + a.tr_off[m], params + s.off[m], s.rows[m], s.cols[m], true);
        }
        __syncthreads();
    }
    auto image = [&](int m, bool tr) -> const _Float16 * {
        if (a.resident) return lds + (tr ? a.tr_off[m] : a.fwd_off[m]);
        __syncthreads();
        stage_image(lds, params + s.off[m], s.rows[m], s.cols[m], tr);
        __syncthreads();
        return lds;
    };
    float4v dw[SLOTS] = {};
    const int64_t nblk = (n + kMlpRowsPerBlock - 1) / kMlpRowsPerBlock;
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {          // uniform over the workgroup
        const int64_t row = blk * kMlpRowsPerBlock + col;
        // forward, keeping every hidden activation on a stack: a_L on top, a_1 at depth L - 1
        half8 hs[kMlpMaxHidden][KS];
        half8 h[KS];
        {
            const _Float16 *img = image(0, false);
            float4v acc[NT] = {};
            for (int ks = 0; ks < ks0; ++ks) {
                const half8 b = load_x(x, row, n, s, a.vec, ks, q);
#pragma unroll
                for (int rt = 0; rt < NT; ++rt) acc[rt] = mfma(frag(img, rt, ks0, ks, lane), b, acc[rt]);
            }
            pack(acc, h, s.act);
            push(hs, h);
        }
        for (int m = 1; m < L; ++m) {
            const _Float16 *img = image(m, false);
            float4v acc[NT] = {};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                for (int rt = 0; rt < NT; ++rt) acc[rt] = mfma(frag(img, rt, KS, ks, lane), h[ks], acc[rt]);
            pack(acc, h, s.act);
            push(hs, h);
        }
        // delta of the output: fp16(S * dy * out_act'(z)); padded output rows get 0
        half8 d[KD];
        {
            float4v dt[4] = {};
            const _Float16 *img = image(L, false);
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) {
                if (rt >= nto) break;
                float4v z = {};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) z = mfma(frag(img, rt, KS, ks, lane), h[ks], z);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int c = 16 * rt + 4 * q + r;
                    float g = (row < n && c < s.n_out) ? dy[row * s.n_out + c] : 0.0f;
                    g *= kMlpLossScale;
                    if (s.out_act == kActSigmoid) {
                        const float yv = sigmoid(z[r]);
                        g *= yv * (1.0f - yv);
                    }
                    dt[rt][r] = g;
                }
            }
            pack(dt, d, kActNone);
        }
        // down the network: matrix m's dW (if in this pass's group), then the delta of matrix m - 1, or dx
        for (int m = L; m >= a.down_to; --m) {
            if (m > 0) pop(hs, h);                                          // a_m, the input of matrix m
            if (m >= a.lo && m <= a.hi) {
                __syncthreads();                                            // the previous matrix's images are consumed
#pragma unroll
                for (int ks = 0; ks < KD; ++ks)
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int i = 32 * ks + kmap(j, q);
                        if (i < s.rows[m]) img_d[i * kMlpImageStride + col] = d[ks][j];
                    }
                if (m == 0) {
                    for (int ks = 0; ks < ks0; ++ks) {
                        const half8 b = load_x(x, row, n, s, a.vec, ks, q);
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const int k = 32 * ks + kmap(j, q);
                            if (k < s.in_w) img_a[k * kMlpImageStride + col] = b[j];
                        }
                    }
                } else {
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const int k = 32 * ks + kmap(j, q);
                            if (k < W) img_a[k * kMlpImageStride + col] = h[ks][j];
                        }
                }
                __syncthreads();
                const int t0 = a.tile_off[m], t1 = a.tile_off[m + 1], nct = s.cols[m] / 16;
#pragma unroll
                for (int sl = 0; sl < SLOTS; ++sl) {
                    const int tau = sl * 4 + wave;
                    if (tau >= t0 && tau < t1) {
                        const int t = tau - t0, rt = t / nct, ct = t - rt * nct;
#pragma unroll
                        for (int kb = 0; kb < kMlpRowsPerBlock / 32; ++kb) {
                            const half8 A = *reinterpret_cast<const half8 *>(img_d + (16 * rt + (lane & 15)) * kMlpImageStride + 32 * kb + 8 * q);
                            const half8 B = *reinterpret_cast<const half8 *>(img_a + (16 * ct + (lane & 15)) * kMlpImageStride + 32 * kb + 8 * q);
                            dw[sl] = mfma(A, B, dw[sl]);
                        }
                    }
                }
            }
            if (m > a.down_to) {
                // delta_{m-1}^T = (W_m^T . delta_m^T) * act'(a_m), act' from the stored fp16 a_m
                const _Float16 *img = image(m, true);
                const int nks = (s.rows[m] + 31) / 32;
                float4v acc[NT] = {};
#pragma unroll
                for (int ks = 0; ks < KD; ++ks) {
                    if (ks >= nks) break;
#pragma unroll
                    for (int rt = 0; rt < NT; ++rt) acc[rt] = mfma(frag(img, rt, nks, ks, lane), d[ks], acc[rt]);
                }
#pragma unroll
                for (int ks = 0; ks < KD; ++ks)
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int t = 2 * ks + (j >> 2);
                        const float v = t < NT ? acc[t < NT ? t : 0][j & 3] : 0.0f;
                        const bool live = ks < KS && (s.act != kActRelu || h[ks < KS ? ks : 0][j] > static_cast<_Float16>(0.0f));
                        d[ks][j] = live ? static_cast<_Float16>(v) : static_cast<_Float16>(0.0f);
                    }
            } else if (m == 0 && a.want_dx) {
                // dx = W_0^T . delta_0^T / S on the real input columns
                const _Float16 *img = image(0, true);
                for (int rt = 0; rt < s.in_w / 16; ++rt) {
                    float4v acc = {};
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) acc = mfma(frag(img, rt, KS, ks, lane), d[ks], acc);
                    if (row < n) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int c = 16 * rt + 4 * q + r;
                            if (c < s.n_in) grad_x[row * s.n_in + c] = acc[r] * (1.0f / kMlpLossScale);
                        }
                    }
                }
            }
        }
    }
    // this workgroup's partial of every dW tile of the pass: D column lane & 15 = input neuron, row 4 q + reg = output neuron
    float *wp = ws + int64_t(blockIdx.x) * s.n_params;
#pragma unroll
    for (int sl = 0; sl < SLOTS; ++sl) {
        const int tau = sl * 4 + wave;
        if (tau >= a.n_tiles) continue;
        int m = a.lo;
        while (tau >= a.tile_off[m + 1]) ++m;
        const int t = tau - a.tile_off[m], nct = s.cols[m] / 16, rt = t / nct, ct = t - rt * nct;
#pragma unroll
        for (int r = 0; r < 4; ++r) wp[s.off[m] + int64_t(16 * rt + 4 * q + r) * s.cols[m] + 16 * ct + (lane & 15)] = dw[sl][r];
    }
}

// grad[p] = (sum over workgroups g = 0, 1, ... of ws[g][p]) / S
__global__ __launch_bounds__(kThreads) void mlp_reduce_kernel(const float *__restrict__ ws, int64_t n_params, int64_t n_blocks,
                                                              float *__restrict__ grad)
{
    const int64_t p = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (p >= n_params) return;
    float acc = 0.0f;
    for (int64_t g = 0; g < n_blocks; ++g) acc += ws[g * n_params + p];
    grad[p] = acc * (1.0f / kMlpLossScale);
}

// bytes of the A-operand fragment image of matrix m (tr: of its transpose)
int image_halfs(const MlpShape &s, int m, bool tr)
{
    const int rows = tr ? s.cols[m] : s.rows[m], cols = tr ? s.rows[m] : s.cols[m];
    return (rows / 16) * ((cols + 31) / 32) * 64 * 8;
}

int slots_for(const MlpShape &s)
{
    int tiles = 0;
    for (int m = 0; m <= s.n_hidden; ++m) tiles += (s.rows[m] / 16) * (s.cols[m] / 16);
    return tiles <= 4 * 8 ? 8 : 32;
}

template <int W>
hipError_t forward_w(const float *x, int64_t n, const float *params, const MlpArgs &a, int lds_halfs, float *y, hipStream_t stream)
{
    const int64_t nblk = (n + kMlpRowsPerBlock - 1) / kMlpRowsPerBlock;
    const int grid = int(nblk < kFwdMaxBlocks ? nblk : kFwdMaxBlocks);
    const size_t bytes = size_t(lds_halfs) * 2;
    if (bytes > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&mlp_forward_kernel<W>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, int(bytes));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(mlp_forward_kernel<W>, dim3(grid), dim3(kThreads), bytes, stream, x, n, params, a, y);
    return hipGetLastError();
}

template <int W, int SLOTS>
hipError_t backward_w(const float *x, int64_t n, const float *params, const MlpArgs &a, int lds_halfs, int64_t grid, const float *dy,
                      float *grad_x, float *ws, hipStream_t stream)
{
    const size_t bytes = size_t(lds_halfs) * 2;
    if (bytes > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&mlp_backward_kernel<W, SLOTS>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, int(bytes));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((mlp_backward_kernel<W, SLOTS>), dim3(unsigned(grid)), dim3(kThreads), bytes, stream, x, n, params, a, dy, grad_x, ws);
    return hipGetLastError();
}

}  // namespace

int64_t mlp_backward_blocks(const MlpShape &s, int64_t n_rows)
{
    const int64_t nblk = (n_rows + kMlpRowsPerBlock - 1) / kMlpRowsPerBlock;
    const int64_t cap = slots_for(s) == 8 ? 512 : 256;
    return nblk < cap ? nblk : cap;
}

int64_t mlp_workspace_bytes(const MlpShape &s, int64_t n_rows)
{
    return n_rows <= 0 ? 0 : mlp_backward_blocks(s, n_rows) * s.n_params * int64_t(sizeof(float));
}

hipError_t launch_mlp_forward(const float *x, int64_t n, const float *params, const MlpShape &s, float *y, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    MlpArgs a{};
    a.s = s;
    a.vec = (s.n_in % 4 == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0) ? 1 : 0;
    int total = 0, biggest = 0;
    for (int m = 0; m <= s.n_hidden; ++m) {
        a.fwd_off[m] = total;
        total += image_halfs(s, m, false);
        biggest = image_halfs(s, m, false) > biggest ? image_halfs(s, m, false) : biggest;
    }
    a.resident = total * 2 <= kMlpResidentBytes;
    const int lds = a.resident ? total : biggest;
    switch (s.width) {
    case 16: return forward_w<16>(x, n, params, a, lds, y, stream);
    case 32: return forward_w<32>(x, n, params, a, lds, y, stream);
    case 64: return forward_w<64>(x, n, params, a, lds, y, stream);
    default: return forward_w<128>(x, n, params, a, lds, y, stream);
    }
}

hipError_t launch_mlp_backward(const float *x, int64_t n, const float *params, const MlpShape &s, const float *dy, float *grad_params,
                               float *grad_x, float *workspace, hipStream_t stream)
{
    if (n <= 0 || (!grad_params && !grad_x)) return hipSuccess;
    const int L = s.n_hidden, slots = slots_for(s);
    MlpArgs a{};
    a.s = s;
    a.vec = (s.n_in % 4 == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0) ? 1 : 0;
    int total = 0, biggest = 0;
    for (int m = 0; m <= L; ++m) {
        const int f = image_halfs(s, m, false), t = image_halfs(s, m, true);
        a.fwd_off[m] = total;
        a.tr_off[m] = total + f;
        total += f + t;
        biggest = f > biggest ? f : biggest;
        biggest = t > biggest ? t : biggest;
    }
    a.resident = total * 2 <= kMlpResidentBytes;
    int kmax = s.in_w > s.width ? s.in_w : s.width, rmax = s.out_w > s.width ? s.out_w : s.width;
    a.img_off = a.resident ? total : biggest;
    a.img_a_off = a.img_off + rmax * kMlpImageStride;
    const int lds = a.img_a_off + kmax * kMlpImageStride;
    const int64_t grid = mlp_backward_blocks(s, n);

    // passes: consecutive matrices while their tiles fit 4 waves x slots (one pass without dW when grad_params is NULL)
    int m0 = 0;
    while (true) {
        int m1 = m0 - 1, tiles = 0;
        a.tile_off[m0] = 0;
        if (grad_params) {
            while (m1 + 1 <= L) {
                const int t = (s.rows[m1 + 1] / 16) * (s.cols[m1 + 1] / 16);
                if (tiles + t > 4 * slots) break;
                ++m1;
                tiles += t;
                a.tile_off[m1 + 1] = tiles;
            }
        }
        a.lo = grad_params ? m0 : L + 1;
        a.hi = grad_params ? m1 : L;
        a.n_tiles = tiles;
        a.want_dx = grad_x && (!grad_params || m0 == 0);
        a.down_to = a.want_dx ? 0 : a.lo;
        hipError_t e;
        switch (s.width * 100 + slots) {
        case 1608: e = backward_w<16, 8>(x, n, params, a, lds, grid, dy, grad_x, workspace, stream); break;
        case 1632: e = backward_w<16, 32>(x, n, params, a, lds, grid, dy, grad_x, workspace, stream); break;
        case 3208: e = backward_w<32, 8>(x, n, params, a, lds, grid, dy, grad_x, workspace, stream); break;
        case 3232: e = backward_w<32, 32>(x, n, params, a, lds, grid, dy, grad_x, workspace, stream); break;
        case 6408: e = backward_w<64, 8>(x, n, params, a, lds, grid, dy, grad_x, workspace, stream); break;
        case 6432: e = backward_w<64, 32>(x, n, params, a, lds, grid, dy, grad_x, workspace, stream); break;
        case 12808: e = backward_w<128, 8>(x, n, params, a, lds, grid, dy, grad_x, workspace, stream); break;
        default: e = backward_w<128, 32>(x, n, params, a, lds, grid, dy, grad_x, workspace, stream); break;
        }
        if (e != hipSuccess) return e;
        if (!grad_params || m1 >= L) break;
        m0 = m1 + 1;
    }
    if (grad_params) {
        const int64_t blocks = (s.n_params + kThreads - 1) / kThreads;
        hipLaunchKernelGGL(mlp_reduce_kernel, dim3(unsigned(blocks)), dim3(kThreads), 0, stream, workspace, s.n_params, grid, grad_params);
        return hipGetLastError();
    }
    return hipSuccess;
}

}  // namespace tsamd
