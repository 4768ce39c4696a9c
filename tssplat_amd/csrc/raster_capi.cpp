// C ABI of the renderer slice (include/tssplat_amd.h, "renderer" section): stateless entry points, the caller owns
// every buffer (positions, triangles, the depth-key workspace, outputs) and names the device by making it current.
#include "capi_common.h"
#include "raster.h"

using tsamd::capi_fail;
using tsamd::check_not_null;
using tsamd::pixel_count;

namespace {

int check_image(int64_t batch, int32_t height, int32_t width) { return tsamd::check_image(batch, height, width, false); }

// the sizes of tsamd_rasterize and of the alpha stage, which bins triangles the same way
int check_render(int64_t batch, int64_t n_vertices, int64_t n_triangles, int32_t height, int32_t width)
{
    const int rc = check_image(batch, height, width);
    return rc ? rc : tsamd::check_mesh_sizes(n_vertices, n_triangles, batch, true);
}

}  // namespace

extern "C" {

int64_t tsamd_rasterize_workspace_bytes(int64_t batch, int64_t n_vertices, int32_t height, int32_t width)
{
    if (batch < 0 || n_vertices < 0 || height < 0 || width < 0) return -1;
    // depth keys (padded to 16 B) + snapped vertices + one flag per view (has a vertex at w <= 0: near-plane clipping needed)
    return ((pixel_count(batch, height, width) + 1) & ~int64_t(1)) * 8 + batch * n_vertices * 16 + ((batch * 4 + 15) & ~int64_t(15));
}

int64_t tsamd_pair_masks_bytes(int64_t batch, int32_t height, int32_t width)
{
    if (check_image(batch, height, width) != TSAMD_OK) return -1;
    return tsamd::pair_masks_bytes(batch, height, width);
}

int tsamd_rasterize(const float *pos_clip_dev, int64_t batch, int64_t n_vertices, const int32_t *tri_dev, int64_t n_triangles, int32_t height,
                    int32_t width, void *workspace_dev, float *rast_out_dev, void *pair_masks_out_dev, void *stream)
{
    int rc = check_render(batch, n_vertices, n_triangles, height, width);
    if (rc) return rc;
    if (pixel_count(batch, height, width) > 0 && (rc = check_not_null({{workspace_dev, "workspace_dev"}, {rast_out_dev, "rast_out_dev"}}))) return rc;
    if (batch * n_triangles > 0 && (rc = check_not_null({{pos_clip_dev, "pos_clip_dev"}, {tri_dev, "tri_dev"}}))) return rc;
    TSAMD_HIP(tsamd::launch_rasterize(pos_clip_dev, batch, n_vertices, tri_dev, n_triangles, height, width, workspace_dev, rast_out_dev,
                                      pair_masks_out_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_interpolate(const float *attr_dev, int64_t attr_batch, int64_t n_vertices, int32_t n_channels, const float *rast_dev,
                      const int32_t *tri_dev, int64_t n_triangles, int64_t batch, int32_t height, int32_t width, float *out_dev, void *stream)
{
    int rc = check_image(batch, height, width);
    if (rc) return rc;
    if (n_vertices < 0 || n_triangles < 0 || n_channels < 1 || (attr_batch != 1 && attr_batch != batch))
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "attr_batch must be 1 or batch, n_channels >= 1, sizes >= 0");
    const int64_t pixels = pixel_count(batch, height, width);
    if (pixels > 0 && (rc = check_not_null({{rast_dev, "rast_dev"}, {out_dev, "out_dev"}}))) return rc;
    if (pixels > 0 && n_triangles > 0 && (rc = check_not_null({{attr_dev, "attr_dev"}, {tri_dev, "tri_dev"}}))) return rc;
    TSAMD_HIP(tsamd::launch_interpolate(attr_dev, attr_batch, n_vertices, n_channels, rast_dev, tri_dev, n_triangles, batch, height, width, out_dev,
                                        static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_interpolate_backward(const float *attr_dev, int64_t attr_batch, int64_t n_vertices, int32_t n_channels, const float *rast_dev,
                               const int32_t *tri_dev, int64_t n_triangles, int64_t batch, int32_t height, int32_t width, const float *grad_out_dev,
                               float *grad_attr_dev, float *grad_rast_dev, void *stream)
{
    int rc = check_image(batch, height, width);
    if (rc) return rc;
    if (n_vertices < 0 || n_triangles < 0 || n_channels < 1 || (attr_batch != 1 && attr_batch != batch))
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "attr_batch must be 1 or batch, n_channels >= 1, sizes >= 0");
    const int64_t pixels = pixel_count(batch, height, width);
    if (attr_batch * n_vertices > 0 && !grad_attr_dev) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grad_attr_dev is null");
    if (pixels > 0 && (rc = check_not_null({{rast_dev, "rast_dev"}, {grad_out_dev, "grad_out_dev"}}))) return rc;
    if (pixels > 0 && n_triangles > 0 && (rc = check_not_null({{attr_dev, "attr_dev"}, {tri_dev, "tri_dev"}}))) return rc;
    TSAMD_HIP(tsamd::launch_interpolate_backward(attr_dev, attr_batch, n_vertices, n_channels, rast_dev, tri_dev, n_triangles, batch, height, width,
                                                 grad_out_dev, grad_attr_dev, grad_rast_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_rasterize_backward(const float *pos_clip_dev, int64_t batch, int64_t n_vertices, const int32_t *tri_dev, int64_t n_triangles,
                             int32_t height, int32_t width, const float *rast_dev, const float *grad_rast_dev, float *grad_pos_dev, void *stream)
{
    int rc = check_image(batch, height, width);
    if (rc) return rc;
    if (n_vertices < 0 || n_triangles < 0) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "negative size");
    if (batch * n_vertices > 0 && !grad_pos_dev) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grad_pos_dev is null");
    if (pixel_count(batch, height, width) > 0 && n_triangles > 0 &&
        (rc = check_not_null({{pos_clip_dev, "pos_clip_dev"}, {tri_dev, "tri_dev"}, {rast_dev, "rast_dev"}, {grad_rast_dev, "grad_rast_dev"}})))
        return rc;
    TSAMD_HIP(tsamd::launch_rasterize_backward(pos_clip_dev, batch, n_vertices, tri_dev, n_triangles, height, width, rast_dev, grad_rast_dev,
                                               grad_pos_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int64_t tsamd_antialias_topology_workspace_bytes(int64_t n_triangles)
{
    if (n_triangles < 0 || n_triangles >= (int64_t(1) << 30)) return -1;   // (triangle, edge) ids are 32-bit
    return tsamd::antialias_topology_workspace_bytes(n_triangles);
}

int tsamd_antialias_topology(const int32_t *tri_dev, int64_t n_triangles, void *workspace_dev, int32_t *edge_partner_dev, void *stream)
{
    if (n_triangles < 0 || n_triangles >= (int64_t(1) << 30)) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "n_triangles out of range (0 .. 2^30 - 1)");
    if (n_triangles > 0) {
        const int rc = check_not_null({{tri_dev, "tri_dev"}, {workspace_dev, "workspace_dev"}, {edge_partner_dev, "edge_partner_dev"}});
        if (rc) return rc;
    }
    TSAMD_HIP(tsamd::launch_antialias_topology(tri_dev, n_triangles, workspace_dev, edge_partner_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

namespace {
int check_antialias(int64_t batch, int64_t n_vertices, int64_t n_triangles, int32_t height, int32_t width, int32_t n_channels)
{
    int rc = check_image(batch, height, width);
    if (rc) return rc;
    if (n_vertices < 0 || n_triangles < 0 || n_channels < 1) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "negative size or n_channels < 1");
    return TSAMD_OK;
}
}  // namespace

int64_t tsamd_antialias_prepared_bytes(int64_t batch, int64_t n_vertices, int64_t n_triangles, int32_t height, int32_t width)
{
    if (check_image(batch, height, width) != TSAMD_OK || n_vertices < 0 || n_triangles < 0) return -1;
    return tsamd::antialias_prepared_bytes(batch, n_vertices, n_triangles, height, width);
}

int tsamd_antialias_prepare(const float *rast_dev, const float *pos_clip_dev, const int32_t *tri_dev, const int32_t *edge_partner_dev,
                            const void *pair_masks_dev, int64_t batch, int64_t n_vertices, int64_t n_triangles, int32_t height, int32_t width,
                            void *prepared_dev, void *stream)
{
    int rc = check_antialias(batch, n_vertices, n_triangles, height, width, 1);
    if (rc) return rc;
    const int64_t pixels = pixel_count(batch, height, width);
    if ((pixels > 0 || batch * n_vertices > 0) && !prepared_dev) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "prepared_dev is null");
    if (pixels > 0 && !rast_dev && !pair_masks_dev) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "without pair_masks_dev, rast_dev is null");
    if (batch * n_vertices > 0 && !pos_clip_dev) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "pos_clip_dev is null");
    if (batch * n_triangles > 0 && (rc = check_not_null({{tri_dev, "tri_dev"}, {edge_partner_dev, "edge_partner_dev"}}))) return rc;
    TSAMD_HIP(tsamd::launch_antialias_prepare(rast_dev, pos_clip_dev, tri_dev, edge_partner_dev, pair_masks_dev, batch, n_vertices, n_triangles, height, width,
                                              prepared_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_antialias(const float *color_dev, const float *rast_dev, const float *pos_clip_dev, const void *prepared_dev, const int32_t *tri_dev,
                    const int32_t *edge_partner_dev, int64_t batch, int64_t n_vertices, int64_t n_triangles, int32_t height, int32_t width, int32_t n_channels, float *out_dev,
                    void *stream)
{
    int rc = check_antialias(batch, n_vertices, n_triangles, height, width, n_channels);
    if (rc) return rc;
    const int64_t pixels = pixel_count(batch, height, width);
    if (pixels > 0 && (rc = check_not_null({{color_dev, "color_dev"}, {rast_dev, "rast_dev"}, {out_dev, "out_dev"}}))) return rc;
    if (pixels > 0 && n_triangles > 0 && (rc = check_not_null({{pos_clip_dev, "pos_clip_dev"}, {tri_dev, "tri_dev"}, {edge_partner_dev, "edge_partner_dev"}}))) return rc;
    TSAMD_HIP(tsamd::launch_antialias(color_dev, rast_dev, pos_clip_dev, prepared_dev, tri_dev, edge_partner_dev, batch, n_vertices, n_triangles, height, width,
                                      n_channels, out_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_antialias_backward(const float *color_dev, const float *rast_dev, const float *pos_clip_dev, const void *prepared_dev,
                             const int32_t *tri_dev, const int32_t *edge_partner_dev, int64_t batch, int64_t n_vertices, int64_t n_triangles, int32_t height, int32_t width,
                             int32_t n_channels, const float *grad_out_dev, float pos_gradient_boost, float *grad_color_dev, float *grad_pos_dev,
                             void *stream)
{
    int rc = check_antialias(batch, n_vertices, n_triangles, height, width, n_channels);
    if (rc) return rc;
    const int64_t pixels = pixel_count(batch, height, width);
    if (!grad_color_dev && !grad_pos_dev) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grad_color_dev and grad_pos_dev are both null");
    if (pixels > 0 && (rc = check_not_null({{color_dev, "color_dev"}, {rast_dev, "rast_dev"}, {grad_out_dev, "grad_out_dev"}}))) return rc;
    if (pixels > 0 && n_triangles > 0 && (rc = check_not_null({{pos_clip_dev, "pos_clip_dev"}, {tri_dev, "tri_dev"}, {edge_partner_dev, "edge_partner_dev"}}))) return rc;
    TSAMD_HIP(tsamd::launch_antialias_backward(color_dev, rast_dev, pos_clip_dev, prepared_dev, tri_dev, edge_partner_dev, batch, n_vertices, n_triangles, height,
                                               width, n_channels, grad_out_dev, pos_gradient_boost, grad_color_dev, grad_pos_dev,
                                               static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

namespace {
// the arguments the two backward calls of tsamd_silhouette share
int check_silhouette_backward(const float *pos_clip_dev, int64_t batch, int64_t n_vertices, const int32_t *tri_dev, int64_t n_triangles,
                              const int32_t *edge_partner_dev, int32_t height, int32_t width, const int32_t *ids_dev, const void *cover_masks_dev,
                              const float *grad_pos_dev)
{
    int rc = check_render(batch, n_vertices, n_triangles, height, width);
    if (rc) return rc;
    if (batch * n_vertices > 0 && !grad_pos_dev) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grad_pos_dev is null");
    if (pixel_count(batch, height, width) <= 0 || batch * n_triangles <= 0) return TSAMD_OK;
    return check_not_null({{ids_dev, "ids_dev"}, {cover_masks_dev, "cover_masks_dev"}, {pos_clip_dev, "pos_clip_dev"}, {tri_dev, "tri_dev"},
                           {edge_partner_dev, "edge_partner_dev"}});
}
}  // namespace

int tsamd_silhouette(const float *pos_clip_dev, int64_t batch, int64_t n_vertices, const int32_t *tri_dev, int64_t n_triangles,
                     const int32_t *edge_partner_dev, int32_t height, int32_t width, void *workspace_dev, int32_t *ids_out_dev, void *cover_masks_out_dev,
                     float *alpha_out_dev, void *stream)
{
    int rc = check_render(batch, n_vertices, n_triangles, height, width);
    if (rc) return rc;
    if (pixel_count(batch, height, width) > 0 && (rc = check_not_null({{workspace_dev, "workspace_dev"}, {ids_out_dev, "ids_out_dev"}, {cover_masks_out_dev, "cover_masks_out_dev"},
                                            {alpha_out_dev, "alpha_out_dev"}})))
        return rc;
    if (batch * n_triangles > 0 && (rc = check_not_null({{pos_clip_dev, "pos_clip_dev"}, {tri_dev, "tri_dev"}, {edge_partner_dev, "edge_partner_dev"}}))) return rc;
    TSAMD_HIP(tsamd::launch_silhouette_cover(pos_clip_dev, batch, n_vertices, tri_dev, n_triangles, height, width, workspace_dev, ids_out_dev,
                                             cover_masks_out_dev, alpha_out_dev, static_cast<hipStream_t>(stream)));
    TSAMD_HIP(tsamd::launch_silhouette_blend(pos_clip_dev, tri_dev, edge_partner_dev, batch, n_vertices, n_triangles, height, width, ids_out_dev,
                                             cover_masks_out_dev, alpha_out_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_silhouette_backward(const float *pos_clip_dev, int64_t batch, int64_t n_vertices, const int32_t *tri_dev, int64_t n_triangles,
                              const int32_t *edge_partner_dev, int32_t height, int32_t width, const int32_t *ids_dev, const void *cover_masks_dev,
                              const float *grad_alpha_dev, float pos_gradient_boost, float *grad_pos_dev, void *stream)
{
    int rc = check_silhouette_backward(pos_clip_dev, batch, n_vertices, tri_dev, n_triangles, edge_partner_dev, height, width, ids_dev, cover_masks_dev,
                                       grad_pos_dev);
    if (rc) return rc;
    if (pixel_count(batch, height, width) > 0 && batch * n_triangles > 0 && !grad_alpha_dev) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grad_alpha_dev is null");
    TSAMD_HIP(tsamd::launch_silhouette_backward(pos_clip_dev, tri_dev, edge_partner_dev, batch, n_vertices, n_triangles, height, width, ids_dev, cover_masks_dev,
                                                grad_alpha_dev, nullptr, nullptr, nullptr, pos_gradient_boost, grad_pos_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int64_t tsamd_silhouette_mse_workspace_bytes(int64_t n)
{
    if (n < 0) return -1;
    return tsamd::silhouette_mse_workspace_bytes(n);
}

int tsamd_silhouette_mse(const float *alpha_dev, const float *target_dev, int64_t n, void *workspace_dev, float *loss_out_dev, void *stream)
{
    if (n < 0) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "negative size");
    if (!loss_out_dev) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "loss_out_dev is null");
    if (n > 0) {
        const int rc = check_not_null({{alpha_dev, "alpha_dev"}, {target_dev, "target_dev"}, {workspace_dev, "workspace_dev"}});
        if (rc) return rc;
    }
    TSAMD_HIP(tsamd::launch_silhouette_mse(alpha_dev, target_dev, n, workspace_dev, loss_out_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_silhouette_mse_backward(const float *pos_clip_dev, int64_t batch, int64_t n_vertices, const int32_t *tri_dev, int64_t n_triangles,
                                  const int32_t *edge_partner_dev, int32_t height, int32_t width, const int32_t *ids_dev, const void *cover_masks_dev,
                                  const float *alpha_dev, const float *target_dev, const float *grad_loss_dev, float pos_gradient_boost, float *grad_pos_dev,
                                  void *stream)
{
    int rc = check_silhouette_backward(pos_clip_dev, batch, n_vertices, tri_dev, n_triangles, edge_partner_dev, height, width, ids_dev, cover_masks_dev,
                                       grad_pos_dev);
    if (rc) return rc;
    if (pixel_count(batch, height, width) > 0 && batch * n_triangles > 0 &&
        (rc = check_not_null({{alpha_dev, "alpha_dev"}, {target_dev, "target_dev"}, {grad_loss_dev, "grad_loss_dev"}})))
        return rc;
    TSAMD_HIP(tsamd::launch_silhouette_backward(pos_clip_dev, tri_dev, edge_partner_dev, batch, n_vertices, n_triangles, height, width, ids_dev, cover_masks_dev,
                                                nullptr, alpha_dev, target_dev, grad_loss_dev, pos_gradient_boost, grad_pos_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

namespace {
struct Output {
    const void *ptr;
    const char *name;
    int64_t elements;
};

// The argument checks of the entry points of the id-driven terms (depth, normal), in the order all four make them: the sizes; with a
// pixel and a triangle (else no kernel runs) the shared pointers, the term's own (`term`, which the entry points take between ids_dev
// and target_dev), target and mask; every output whose array has elements; with a pixel and a triangle again, `last` (the workspace
// of a forward call, the upstream gradient of a backward one).
int check_term(const float *pos_clip_dev, int64_t batch, int64_t n_vertices, const int32_t *tri_dev, int64_t n_triangles, int32_t height, int32_t width,
               const int32_t *ids_dev, std::initializer_list<tsamd::NamedPtr> term, const float *target_dev, const float *mask_dev,
               std::initializer_list<Output> outputs, tsamd::NamedPtr last)
{
    int rc = check_render(batch, n_vertices, n_triangles, height, width);
    if (rc) return rc;
    const bool runs = pixel_count(batch, height, width) > 0 && n_triangles > 0;
    if (runs && ((rc = check_not_null({{pos_clip_dev, "pos_clip_dev"}, {tri_dev, "tri_dev"}, {ids_dev, "ids_dev"}})) || (rc = check_not_null(term)) ||
                 (rc = check_not_null({{target_dev, "target_dev"}, {mask_dev, "mask_dev"}}))))
        return rc;
    for (const Output &o : outputs)
        if (o.elements > 0 && (rc = check_not_null({{o.ptr, o.name}}))) return rc;
    return runs ? check_not_null({last}) : TSAMD_OK;
}
}  // namespace

int64_t tsamd_depth_mse_workspace_bytes(int64_t n)
{
    if (n < 0) return -1;
    return tsamd::depth_mse_workspace_bytes(n);
}

int64_t tsamd_normal_mse_workspace_bytes(int64_t n)
{
    if (n < 0) return -1;
    return tsamd::normal_mse_workspace_bytes(n);
}

int tsamd_depth_mse(const float *pos_clip_dev, int64_t batch, int64_t n_vertices, const int32_t *tri_dev, int64_t n_triangles, int32_t height, int32_t width,
                    const int32_t *ids_dev, const float *world_pos_dev, const float *campos_dev, const float *target_dev, const float *mask_dev,
                    void *workspace_dev, float *loss_out_dev, float *depth_out_dev, void *stream)
{
    const int rc = check_term(pos_clip_dev, batch, n_vertices, tri_dev, n_triangles, height, width, ids_dev, {{world_pos_dev, "world_pos_dev"}, {campos_dev, "campos_dev"}},
                              target_dev, mask_dev, {{loss_out_dev, "loss_out_dev", 1}}, {workspace_dev, "workspace_dev"});   // (the loss is stored even of nothing)
    if (rc) return rc;
    TSAMD_HIP(tsamd::launch_depth_mse(pos_clip_dev, batch, n_vertices, tri_dev, n_triangles, height, width, ids_dev, world_pos_dev, campos_dev, target_dev, mask_dev,
                                      workspace_dev, loss_out_dev, depth_out_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_depth_mse_backward(const float *pos_clip_dev, int64_t batch, int64_t n_vertices, const int32_t *tri_dev, int64_t n_triangles, int32_t height,
                             int32_t width, const int32_t *ids_dev, const float *world_pos_dev, const float *campos_dev, const float *target_dev,
                             const float *mask_dev, const float *grad_loss_dev, int32_t accumulate_pos, float *grad_world_dev, float *grad_pos_dev, void *stream)
{
    const int rc = check_term(pos_clip_dev, batch, n_vertices, tri_dev, n_triangles, height, width, ids_dev, {{world_pos_dev, "world_pos_dev"}, {campos_dev, "campos_dev"}},
                              target_dev, mask_dev, {{grad_world_dev, "grad_world_dev", n_vertices}, {grad_pos_dev, "grad_pos_dev", batch * n_vertices}},
                              {grad_loss_dev, "grad_loss_dev"});
    if (rc) return rc;
    TSAMD_HIP(tsamd::launch_depth_mse_backward(pos_clip_dev, batch, n_vertices, tri_dev, n_triangles, height, width, ids_dev, world_pos_dev, campos_dev, target_dev,
                                               mask_dev, grad_loss_dev, accumulate_pos, grad_world_dev, grad_pos_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_normal_mse(const float *pos_clip_dev, int64_t batch, int64_t n_vertices, const int32_t *tri_dev, int64_t n_triangles, int32_t height, int32_t width,
                     const int32_t *ids_dev, const float *attr_dev, const float *target_dev, const float *mask_dev, void *workspace_dev, float *loss_out_dev,
                     float *normal_out_dev, void *stream)
{
    const int rc = check_term(pos_clip_dev, batch, n_vertices, tri_dev, n_triangles, height, width, ids_dev, {{attr_dev, "attr_dev"}}, target_dev, mask_dev,
                              {{loss_out_dev, "loss_out_dev", 1}}, {workspace_dev, "workspace_dev"});
    if (rc) return rc;
    TSAMD_HIP(tsamd::launch_normal_mse(pos_clip_dev, batch, n_vertices, tri_dev, n_triangles, height, width, ids_dev, attr_dev, target_dev, mask_dev, workspace_dev,
                                       loss_out_dev, normal_out_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_normal_mse_backward(const float *pos_clip_dev, int64_t batch, int64_t n_vertices, const int32_t *tri_dev, int64_t n_triangles, int32_t height,
                              int32_t width, const int32_t *ids_dev, const float *attr_dev, const float *target_dev, const float *mask_dev,
                              const float *grad_loss_dev, int32_t accumulate_pos, float *grad_attr_dev, float *grad_pos_dev, void *stream)
{
    const int rc = check_term(pos_clip_dev, batch, n_vertices, tri_dev, n_triangles, height, width, ids_dev, {{attr_dev, "attr_dev"}}, target_dev, mask_dev,
                              {{grad_attr_dev, "grad_attr_dev", n_vertices}, {grad_pos_dev, "grad_pos_dev", batch * n_vertices}}, {grad_loss_dev, "grad_loss_dev"});
    if (rc) return rc;
    TSAMD_HIP(tsamd::launch_normal_mse_backward(pos_clip_dev, batch, n_vertices, tri_dev, n_triangles, height, width, ids_dev, attr_dev, target_dev, mask_dev,
                                                grad_loss_dev, accumulate_pos, grad_attr_dev, grad_pos_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

}  // extern "C"
