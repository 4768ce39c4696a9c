// Fully fused MLP (tiny-cuda-nn's FullyFusedMLP / CutlassMLP, bias-free): the colour MLP of the texture stage when its
// mlp_network_config names a tcnn network (models/networks.py:314-339).  Semantics: tests/mlp_oracle.py.
//
// Matrices m = 0 .. L (L = n_hidden_layers): m = 0 is [W, in_w], 1 .. L-1 are [W, W], m = L is [out_w, W], row-major
// [out, in], one after another in one flat float32 vector.  in_w = next_multiple(n_in, 16), out_w = next_multiple(n_out, 16);
// padded input columns read 1.0 (a bias), padded output rows are computed and discarded.  Operands are fp16, sums fp32.
#pragma once

#include <cstdint>
#include <string>

#include <hip/hip_runtime_api.h>

namespace tsamd {

constexpr int kMlpMaxHidden = 8;
constexpr float kMlpLossScale = 128.0f;             // tiny-cuda-nn's torch binding: backward runs on S * dL/dy
constexpr int kMlpRowsPerBlock = 64;                // four waves of 16 rows each
constexpr int kMlpResidentBytes = 64 * 1024;        // a network whose fp16 fragment images fit this is staged once per workgroup
constexpr int kMlpImageStride = 72;                 // halfs per row of the backward's [neuron][row] images (64 rows + 8 pad)

struct MlpShape {
    int32_t width, n_hidden, n_in, n_out, in_w, out_w, act, out_act;
    int64_t n_params;
    int64_t off[kMlpMaxHidden + 2];                 // first float of matrix m; off[L + 1] = n_params
    int32_t rows[kMlpMaxHidden + 1], cols[kMlpMaxHidden + 1];   // matrix m is [rows[m], cols[m]]
};

// Fills `s`; false + `err` on a config outside the envelope (width 16/32/64/128, 1..8 hidden layers, 1..256 inputs,
// 1..64 outputs, activation ReLU/None, output activation None/Sigmoid).
bool mlp_layout(int32_t n_in, int32_t n_out, int32_t width, int32_t n_hidden, int32_t act, int32_t out_act, MlpShape &s,
                std::string &err);
// Workgroups of the backward for n_rows rows (fixed by the config and n_rows alone: the workspace and the summation order
// do not depend on the device).
int64_t mlp_backward_blocks(const MlpShape &s, int64_t n_rows);
int64_t mlp_workspace_bytes(const MlpShape &s, int64_t n_rows);

hipError_t launch_mlp_forward(const float *x, int64_t n, const float *params, const MlpShape &s, float *y, hipStream_t stream);
hipError_t launch_mlp_backward(const float *x, int64_t n, const float *params, const MlpShape &s, const float *dy,
                               float *grad_params, float *grad_x, float *workspace, hipStream_t stream);

}  // namespace tsamd
