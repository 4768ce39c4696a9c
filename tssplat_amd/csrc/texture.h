// The texture side of the renderer slice: the closed-form per-triangle atlas (two mirrored right triangles per square cell),
// the bake of surface positions into it, and dr.texture (nearest / bilinear sampling of a 2-D texture and its backward).
// Semantics: tests/atlas_oracle.py and tests/texture_oracle.py.
#pragma once

#include <cstdint>
#include <string>

#include <hip/hip_runtime_api.h>

namespace tsamd {

// T triangles in a square texture of R texels: n cells per row, c = R / n texels per cell, legs of L = c - 5 texels.
// Passed to the bake kernel by value: the host function below is the only place that computes it.
struct AtlasLayout {
    int32_t cells_per_row;   // n = ceil(sqrt(ceil(T / 2)))
    int32_t cell;            // c
    int32_t leg;             // L
};

constexpr int32_t kAtlasMinCell = 6;       // c >= 6: L >= 1
constexpr int32_t kAtlasMaxRes = 32768;

// Fills `lay` whenever the arguments are in range (n_triangles >= 1, 1 <= texture_res <= kAtlasMaxRes), so that a caller can
// name the smallest workable resolution kAtlasMinCell * n; false + `err` when they are not, or when c < kAtlasMinCell.
bool atlas_layout(int64_t n_triangles, int32_t texture_res, AtlasLayout &lay, std::string &err);

hipError_t launch_atlas_bake_positions(const float *v_pos, int64_t n_vertices, const int32_t *tri, int64_t n_triangles, int32_t texture_res,
                                       const AtlasLayout &lay, float *positions, int32_t *owner, hipStream_t stream);

// filter: 0 nearest, 1 linear; boundary: 0 wrap, 1 clamp, 2 zero (TSAMD_TEX_* of include/tssplat_amd.h)
hipError_t launch_texture(const float *tex, int64_t tex_batch, int32_t tex_h, int32_t tex_w, int32_t channels, const float *uv, int64_t pixels,
                          int64_t pixels_per_image, int filter, int boundary, float *out, hipStream_t stream);
// grad_tex ([tex_batch, tex_h, tex_w, channels], may be null) is zero-filled and accumulated; grad_uv ([pixels, 2], may be null;
// linear only) is written.
hipError_t launch_texture_backward(const float *tex, int64_t tex_batch, int32_t tex_h, int32_t tex_w, int32_t channels, const float *uv,
                                   int64_t pixels, int64_t pixels_per_image, int filter, int boundary, const float *grad_out, float *grad_tex,
                                   float *grad_uv, hipStream_t stream);

}  // namespace tsamd
