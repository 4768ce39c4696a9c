// C ABI of the texture stage's image side (include/tssplat_amd.h, tsamd_shade*): stateless entry points over a caller-owned blend
// plan.  Every argument is checked before the first device call.
#include "capi_common.h"
#include "raster.h"
#include "shade.h"

using tsamd::capi_fail;
using tsamd::check_not_null;
using tsamd::kMaxPixels;
using tsamd::pixel_count;

namespace {

constexpr int64_t kMaxBlends = (int64_t(1) << 31) - 1;   // record offsets and indices are 32-bit, as pixel indices are (kMaxPixels)

int check_image(int64_t batch, int32_t height, int32_t width) { return tsamd::check_image(batch, height, width, true); }
int64_t pixels_of(const tsamd_blend_plan *plan) { return pixel_count(plan->batch, plan->height, plan->width); }

int check_plan_extract(const float *rast_dev, const float *pos_clip_dev, const void *prepared_dev, const int32_t *tri_dev, const int32_t *edge_partner_dev, int64_t batch,
                       int64_t n_vertices, int64_t n_triangles, int32_t height, int32_t width)
{
    int rc = check_image(batch, height, width);
    if (rc || (rc = tsamd::check_mesh_sizes(n_vertices, n_triangles, batch, false))) return rc;
    if (pixel_count(batch, height, width) <= 0 || n_triangles == 0 || n_vertices == 0) return TSAMD_OK;
    return check_not_null({{rast_dev, "rast_dev"}, {pos_clip_dev, "pos_clip_dev"}, {prepared_dev, "prepared_dev"}, {tri_dev, "tri_dev"}, {edge_partner_dev, "edge_partner_dev"}});
}

// the plan itself: sizes, and every array the sizes make the kernels read
int check_plan(const tsamd_blend_plan *plan)
{
    if (!plan) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "plan is null");
    if (plan->struct_size != int32_t(sizeof(tsamd_blend_plan))) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "plan->struct_size is not sizeof(tsamd_blend_plan)");
    int rc = check_image(plan->batch, plan->height, plan->width);
    if (rc) return rc;
    const int64_t pixels = pixels_of(plan);
    if (plan->n_points < 0 || plan->n_points > pixels) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "plan->n_points out of range (0 .. batch x height x width)");
    if (plan->n_blends < 0 || plan->n_blends > 6 * pixels || plan->n_blends > kMaxBlends)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "plan->n_blends out of range (0 .. 6 per pixel, at most 2^31 - 1)");
    if (plan->n_dst < 0 || plan->n_dst > plan->n_blends || plan->n_src < 0 || plan->n_src > plan->n_blends)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "plan->n_dst / n_src out of range (0 .. n_blends)");
    if (pixels > 0 && (rc = check_not_null({{plan->pix_point_dev, "plan->pix_point_dev"}, {plan->pix_dst_dev, "plan->pix_dst_dev"}}))) return rc;
    if (plan->n_points > 0 &&
        (rc = check_not_null({{plan->point_pix_dev, "plan->point_pix_dev"}, {plan->point_dst_dev, "plan->point_dst_dev"}, {plan->point_src_dev, "plan->point_src_dev"}})))
        return rc;
    if (plan->n_blends > 0 &&
        (rc = check_not_null({{plan->dst_ptr_dev, "plan->dst_ptr_dev"}, {plan->dst_src_pix_dev, "plan->dst_src_pix_dev"}, {plan->dst_src_point_dev, "plan->dst_src_point_dev"},
                              {plan->dst_weight_dev, "plan->dst_weight_dev"}, {plan->src_ptr_dev, "plan->src_ptr_dev"}, {plan->src_dst_pix_dev, "plan->src_dst_pix_dev"},
                              {plan->src_dst_slot_dev, "plan->src_dst_slot_dev"}, {plan->src_weight_dev, "plan->src_weight_dev"}})))
        return rc;
    return TSAMD_OK;
}

}  // namespace

extern "C" {

int tsamd_shade_plan_count(const float *rast_dev, const float *pos_clip_dev, const void *prepared_dev, const int32_t *tri_dev, const int32_t *edge_partner_dev,
                           int64_t batch, int64_t n_vertices, int64_t n_triangles, int32_t height, int32_t width, int32_t *counts_out_dev, void *stream)
{
    int rc = check_plan_extract(rast_dev, pos_clip_dev, prepared_dev, tri_dev, edge_partner_dev, batch, n_vertices, n_triangles, height, width);
    if (rc) return rc;
    if (pixel_count(batch, height, width) <= 0) return TSAMD_OK;
    if (!counts_out_dev) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "counts_out_dev is null");
    TSAMD_HIP(tsamd::launch_blend_plan(rast_dev, pos_clip_dev, prepared_dev, tri_dev, edge_partner_dev, batch, n_vertices, n_triangles, height, width, counts_out_dev,
                                       nullptr, 0, nullptr, nullptr, nullptr, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_shade_plan_fill(const float *rast_dev, const float *pos_clip_dev, const void *prepared_dev, const int32_t *tri_dev, const int32_t *edge_partner_dev,
                          int64_t batch, int64_t n_vertices, int64_t n_triangles, int32_t height, int32_t width, const int32_t *offsets_dev, int64_t n_blends,
                          int32_t *dst_out_dev, int32_t *src_out_dev, float *weight_out_dev, void *stream)
{
    int rc = check_plan_extract(rast_dev, pos_clip_dev, prepared_dev, tri_dev, edge_partner_dev, batch, n_vertices, n_triangles, height, width);
    if (rc) return rc;
    if (n_blends < 0 || n_blends > 6 * pixel_count(batch, height, width) || n_blends > kMaxBlends)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "n_blends out of range (0 .. 6 per pixel, at most 2^31 - 1)");
    if (n_blends == 0) return TSAMD_OK;
    if ((rc = check_not_null({{offsets_dev, "offsets_dev"}, {dst_out_dev, "dst_out_dev"}, {src_out_dev, "src_out_dev"}, {weight_out_dev, "weight_out_dev"}}))) return rc;
    TSAMD_HIP(tsamd::launch_blend_plan(rast_dev, pos_clip_dev, prepared_dev, tri_dev, edge_partner_dev, batch, n_vertices, n_triangles, height, width, nullptr,
                                       offsets_dev, n_blends, dst_out_dev, src_out_dev, weight_out_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_shade(const tsamd_blend_plan *plan, const float *color_dev, const float *background_dev, float *out_dev, void *stream)
{
    int rc = check_plan(plan);
    if (rc) return rc;
    if (plan->n_points > 0 && !color_dev) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "color_dev is null");
    if (pixels_of(plan) > 0 && (rc = check_not_null({{background_dev, "background_dev"}, {out_dev, "out_dev"}}))) return rc;
    TSAMD_HIP(tsamd::launch_shade(*plan, color_dev, background_dev, out_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_shade_backward(const tsamd_blend_plan *plan, const float *grad_out_dev, float *grad_color_dev, void *stream)
{
    int rc = check_plan(plan);
    if (rc) return rc;
    if (plan->n_points > 0 && (rc = check_not_null({{grad_out_dev, "grad_out_dev"}, {grad_color_dev, "grad_color_dev"}}))) return rc;
    TSAMD_HIP(tsamd::launch_shade_backward(*plan, grad_out_dev, grad_color_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int64_t tsamd_shade_l1_workspace_bytes(int64_t pixels)
{
    if (pixels < 0 || pixels >= kMaxPixels) return -1;
    return tsamd::shade_l1_workspace_bytes(pixels);
}

int tsamd_shade_l1(const tsamd_blend_plan *plan, const float *color_dev, const float *background_dev, const float *target_dev, int32_t target_channels,
                   void *workspace_dev, float *loss_out_dev, float *image_out_dev, float *point_sign_out_dev, float *dst_sign_out_dev, void *stream)
{
    int rc = check_plan(plan);
    if (rc) return rc;
    if (target_channels != 3 && target_channels != 4) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "target_channels must be 3 or 4");
    if (!loss_out_dev) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "loss_out_dev is null");
    if (plan->n_points > 0 && !color_dev) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "color_dev is null");
    if (pixels_of(plan) > 0 &&
        (rc = check_not_null({{background_dev, "background_dev"}, {target_dev, "target_dev"}, {workspace_dev, "workspace_dev"}})))
        return rc;
    const bool want_signs = point_sign_out_dev || dst_sign_out_dev;
    if (want_signs && ((plan->n_points > 0 && !point_sign_out_dev) || (plan->n_dst > 0 && !dst_sign_out_dev)))
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "point_sign_out_dev and dst_sign_out_dev go together");
    // (a plan without points has nothing to differentiate: the kernel takes point_sign as the switch for both arrays)
    TSAMD_HIP(tsamd::launch_shade_l1(*plan, color_dev, background_dev, target_dev, target_channels, workspace_dev, loss_out_dev, image_out_dev,
                                     plan->n_points > 0 ? point_sign_out_dev : nullptr, dst_sign_out_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_shade_l1_backward(const tsamd_blend_plan *plan, const float *point_sign_dev, const float *dst_sign_dev, const float *grad_loss_dev, float *grad_color_dev,
                            void *stream)
{
    int rc = check_plan(plan);
    if (rc) return rc;
    if (plan->n_points > 0 && (rc = check_not_null({{point_sign_dev, "point_sign_dev"}, {grad_loss_dev, "grad_loss_dev"}, {grad_color_dev, "grad_color_dev"}}))) return rc;
    if (plan->n_points > 0 && plan->n_dst > 0 && !dst_sign_dev) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "dst_sign_dev is null");
    TSAMD_HIP(tsamd::launch_shade_l1_backward(*plan, point_sign_dev, dst_sign_dev, grad_loss_dev, grad_color_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

}  // extern "C"
