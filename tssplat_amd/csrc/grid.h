// Multiresolution hash-grid encoding (Instant-NGP; tiny-cuda-nn's `Grid` encoding, 3-D, trilinear): the colour field of the
// texture stage (materials/explicit_material.py, models/networks.py:97-106).  Semantics: tests/hashgrid_oracle.py.
#pragma once

#include <cstdint>
#include <string>

#include <hip/hip_runtime_api.h>

namespace tsamd {

constexpr int kGridMaxLevels = 32;
// dL/dparams of a level is accumulated in LDS when its table (entries x F x 4 bytes) fits this (gfx950: 160 KB per CU)
constexpr int kGridLdsBytes = 128 * 1024;

// Host-computed per-level table, passed to the kernels by value.
struct GridLevels {
    int64_t offset[kGridMaxLevels];      // first entry of the level (entries, not floats)
    uint32_t entries[kGridMaxLevels];    // the level's entry count (the `% hashmap_size` of grid_index)
    uint32_t res[kGridMaxLevels];
    float scale[kGridMaxLevels];
    uint32_t hashed[kGridMaxLevels];     // 1: coherent prime hash, 0: dense stride index
    int32_t n_levels;
    int32_t lds_levels;                  // levels [0, lds_levels) accumulate dL/dparams in LDS (their table fits)
};

// Fills `lv` (lds_levels = 0) and the total parameter count; false + `err` on a config the encoding does not accept.
bool grid_layout(int32_t n_levels, int32_t n_features, int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale,
                 int32_t dense, GridLevels &lv, int64_t &n_params, std::string &err);

hipError_t launch_grid_encode(const float *x, int64_t n, const float *params, const GridLevels &lv, int32_t n_features, float *out,
                              hipStream_t stream);
hipError_t launch_grid_encode_backward(const float *x, int64_t n, const float *params, const GridLevels &lv, int32_t n_features,
                                       const float *grad_out, float *grad_params, float *grad_x, hipStream_t stream);

}  // namespace tsamd
