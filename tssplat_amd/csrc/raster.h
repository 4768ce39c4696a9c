// Launch interface between the C ABI (raster_capi.cpp) and the renderer-slice kernels (raster_, interpolate_, term_, aa_kernels.hip).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace tsamd {

inline int64_t pixel_count(int64_t batch, int height, int width) { return batch * int64_t(height) * width; }

// workspace: batch * height * width 64-bit depth keys, then batch * n_vertices 16-byte snapped vertices
// pair_masks (optional output, 16 bytes per 64 pixels): see antialias_prepare
hipError_t launch_rasterize(const float *pos_clip, int64_t batch, int64_t n_vertices, const int32_t *tri, int64_t n_tri, int height, int width,
                            void *workspace, float *rast, void *pair_masks, hipStream_t stream);
// grad_pos ([batch, n_vertices, 4]) is zero-filled by the launch
hipError_t launch_rasterize_backward(const float *pos_clip, int64_t batch, int64_t n_vertices, const int32_t *tri, int64_t n_tri, int height, int width,
                                     const float *rast, const float *grad_rast, float *grad_pos, hipStream_t stream);
// antialias (aa_kernels.hip): the edge partner table opp[3 * n_tri] is built once per triangle list
int64_t antialias_topology_workspace_bytes(int64_t n_tri);
hipError_t launch_antialias_topology(const int32_t *tri, int64_t n_tri, void *workspace, int32_t *opp, hipStream_t stream);
// `prepared` (antialias_prepared_bytes): the window coordinates of every (view, vertex) and the mask of pixel pairs with two
// different triangle ids and the per-(view, triangle) edge flags; optional input of the two launches below (null: both computed per use, same operations)
int64_t antialias_prepared_bytes(int64_t batch, int64_t n_vertices, int64_t n_tri, int height, int width);
int64_t pair_masks_bytes(int64_t batch, int height, int width);
// pair_masks: the by-product of launch_rasterize for the same image, or null (then `rast` is scanned for them)
hipError_t launch_antialias_prepare(const float *rast, const float *pos_clip, const int32_t *tri, const int32_t *opp, const void *pair_masks, int64_t batch,
                                    int64_t n_vertices, int64_t n_tri, int height, int width, void *prepared, hipStream_t stream);
hipError_t launch_antialias(const float *color, const float *rast, const float *pos_clip, const void *prepared, const int32_t *tri, const int32_t *opp,
                            int64_t batch, int64_t n_vertices, int64_t n_tri, int height, int width, int channels, float *out, hipStream_t stream);
// grad_color (a copy of grad_out plus the blends' terms) and grad_pos (zero-filled first) may each be null
hipError_t launch_antialias_backward(const float *color, const float *rast, const float *pos_clip, const void *prepared, const int32_t *tri,
                                     const int32_t *opp, int64_t batch, int64_t n_vertices, int64_t n_tri, int height, int width, int channels, const float *grad_out, float boost,
                                     float *grad_color, float *grad_pos, hipStream_t stream);
// The blend plan (tsamd_shade_plan_*, aa_kernels.hip): the blends tsamd_antialias would apply to `rast`, as records.  counts non-null:
// counts[2 pixel + axis] = blends of the pair (zero-filled first).  counts null: the records of every pair from offsets[2 pixel + axis]
// on (the exclusive scan of the counts), pixel indices batch-wide; records at or beyond n_blends are not written.
hipError_t launch_blend_plan(const float *rast, const float *pos_clip, const void *prepared, const int32_t *tri, const int32_t *opp, int64_t batch, int64_t n_vertices,
                             int64_t n_tri, int height, int width, int32_t *counts, const int32_t *offsets, int64_t n_blends, int32_t *rec_dst, int32_t *rec_src,
                             float *rec_weight, hipStream_t stream);
// The alpha stage (tsamd_silhouette*).  cover (raster_kernels.hip): the depth keys of launch_rasterize, then per pixel ids (triangle + 1,
// 0 = background), alpha = 0 / 1 and the coverage masks (pair_masks_bytes; bit = exactly one pixel of the pair is background).
// blend / backward (aa_kernels.hip): the antialias analysis over those masks; backward takes grad_alpha, or (grad_alpha null) alpha,
// target and the device scalar grad_loss of the mean squared error; grad_pos is zero-filled by the launch.
hipError_t launch_silhouette_cover(const float *pos_clip, int64_t batch, int64_t n_vertices, const int32_t *tri, int64_t n_tri, int height, int width,
                                   void *workspace, int32_t *ids, void *cover_masks, float *alpha, hipStream_t stream);
hipError_t launch_silhouette_blend(const float *pos_clip, const int32_t *tri, const int32_t *opp, int64_t batch, int64_t n_vertices, int64_t n_tri, int height, int width,
                                   const int32_t *ids, const void *cover_masks, float *alpha, hipStream_t stream);
hipError_t launch_silhouette_backward(const float *pos_clip, const int32_t *tri, const int32_t *opp, int64_t batch, int64_t n_vertices, int64_t n_tri, int height, int width,
                                      const int32_t *ids, const void *cover_masks, const float *grad_alpha, const float *alpha, const float *target,
                                      const float *grad_loss, float boost, float *grad_pos, hipStream_t stream);
// loss = mean((alpha - target)^2) over n floats, bitwise repeatable; n = 0 stores 0
int64_t silhouette_mse_workspace_bytes(int64_t n);
hipError_t launch_silhouette_mse(const float *alpha, const float *target, int64_t n, void *workspace, float *loss, hipStream_t stream);
// The id-driven image terms (term_kernels.hip): loss = mean over batch * height * width pixels and the term's channels of
// (x_c m - t_c m)^2, x a value of y = interpolate(attr) for attr [n_vertices, 3] from the alpha stage's ids (y = 0 on background), target
// [batch, height, width, channels], mask [batch, height, width]; bitwise repeatable; the output image (optional): x per pixel.  No pixel
// or no triangle: loss 0, nothing else written.  backward: the attribute's gradient [n_vertices, 3] is zero-filled by the launch, grad_pos
// [batch, n_vertices, 4] too unless accumulate_pos != 0 (then it is added to).  n of the workspace sizes is the pixel count.
// The depth term, one channel: x = d = || y - campos[view] || with attr = world_pos (|| campos || on background).
int64_t depth_mse_workspace_bytes(int64_t n);
hipError_t launch_depth_mse(const float *pos_clip, int64_t batch, int64_t n_vertices, const int32_t *tri, int64_t n_tri, int height, int width, const int32_t *ids,
                            const float *world_pos, const float *campos, const float *target, const float *mask, void *workspace, float *loss, float *depth_out,
                            hipStream_t stream);
hipError_t launch_depth_mse_backward(const float *pos_clip, int64_t batch, int64_t n_vertices, const int32_t *tri, int64_t n_tri, int height, int width,
                                     const int32_t *ids, const float *world_pos, const float *campos, const float *target, const float *mask, const float *grad_loss,
                                     int accumulate_pos, float *grad_world, float *grad_pos, hipStream_t stream);
// The normal term, three channels: x = n = y itself.
int64_t normal_mse_workspace_bytes(int64_t n);
hipError_t launch_normal_mse(const float *pos_clip, int64_t batch, int64_t n_vertices, const int32_t *tri, int64_t n_tri, int height, int width, const int32_t *ids,
                             const float *attr, const float *target, const float *mask, void *workspace, float *loss, float *normal_out, hipStream_t stream);
hipError_t launch_normal_mse_backward(const float *pos_clip, int64_t batch, int64_t n_vertices, const int32_t *tri, int64_t n_tri, int height, int width,
                                      const int32_t *ids, const float *attr, const float *target, const float *mask, const float *grad_loss, int accumulate_pos,
                                      float *grad_attr, float *grad_pos, hipStream_t stream);
hipError_t launch_interpolate(const float *attr, int64_t attr_batch, int64_t n_vertices, int channels, const float *rast, const int32_t *tri,
                              int64_t n_tri, int64_t batch, int height, int width, float *out, hipStream_t stream);
// (these two launches: interpolate_kernels.hip)  grad_attr is zero-filled by the launch; grad_rast may be null
hipError_t launch_interpolate_backward(const float *attr, int64_t attr_batch, int64_t n_vertices, int channels, const float *rast, const int32_t *tri,
                                       int64_t n_tri, int64_t batch, int height, int width, const float *grad_out, float *grad_attr, float *grad_rast,
                                       hipStream_t stream);

}  // namespace tsamd
