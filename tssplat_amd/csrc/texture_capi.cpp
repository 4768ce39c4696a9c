// C ABI of the texture side of the renderer slice (include/tssplat_amd.h, "texture atlas and texture sampling" section): the
// host-side atlas layout and the stateless bake / sample / backward entry points.  The caller owns every buffer and names the
// device by making it current.
#include <cstdint>
#include <string>

#include "capi_common.h"
#include "texture.h"

using tsamd::capi_fail;

namespace tsamd {

bool atlas_layout(int64_t n_triangles, int32_t texture_res, AtlasLayout &lay, std::string &err)
{
    lay = AtlasLayout{0, 0, 0};
    if (n_triangles < 1 || n_triangles > (int64_t(1) << 31)) {
        err = "n_triangles must be 1 .. 2^31";
        return false;
    }
    if (texture_res < 1 || texture_res > kAtlasMaxRes) {
        err = "texture_res must be 1 .. " + std::to_string(kAtlasMaxRes);
        return false;
    }
    const int64_t cells = (n_triangles + 1) / 2;
    int64_t n = 1;
    while (n * n < cells) ++n;             // ceil(sqrt(cells)) in integers (n <= 32768)
    lay.cells_per_row = int32_t(n);
    lay.cell = int32_t(texture_res / n);
    lay.leg = lay.cell - 5;
    if (lay.cell < kAtlasMinCell) {
        err = std::to_string(n_triangles) + " triangles need " + std::to_string(n) + " cells per row of at least " + std::to_string(kAtlasMinCell) +
              " texels: texture_res = " + std::to_string(texture_res) + " is too small, the smallest workable one is " +
              std::to_string(kAtlasMinCell * n);
        return false;
    }
    return true;
}

}  // namespace tsamd

namespace {

int check_texture(int64_t tex_batch, int32_t tex_height, int32_t tex_width, int32_t n_channels, int64_t batch, int32_t height, int32_t width,
                  int32_t filter_mode, int32_t boundary_mode)
{
    if (tex_height < 1 || tex_width < 1 || tex_height > tsamd::kAtlasMaxRes || tex_width > tsamd::kAtlasMaxRes || n_channels < 1)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "texture: tex_height / tex_width must be 1 .. 32768 and n_channels >= 1");
    if (batch < 0 || height < 0 || width < 0 || (batch > 0 && int64_t(height) * width > (int64_t(1) << 38) / batch))
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "texture: batch / height / width negative or more than 2^38 output pixels");
    if (tex_batch != 1 && tex_batch != batch) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "texture: tex_batch must be 1 or batch");
    if (filter_mode != TSAMD_TEX_FILTER_NEAREST && filter_mode != TSAMD_TEX_FILTER_LINEAR)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "texture: filter_mode must be TSAMD_TEX_FILTER_NEAREST or TSAMD_TEX_FILTER_LINEAR");
    if (boundary_mode != TSAMD_TEX_BOUNDARY_WRAP && boundary_mode != TSAMD_TEX_BOUNDARY_CLAMP && boundary_mode != TSAMD_TEX_BOUNDARY_ZERO)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "texture: boundary_mode must be TSAMD_TEX_BOUNDARY_WRAP, _CLAMP or _ZERO");
    return TSAMD_OK;
}

}  // namespace

extern "C" {

int tsamd_atlas_layout(int64_t n_triangles, int32_t texture_res, int32_t *cells_per_row_out, int32_t *cell_out, int32_t *leg_out)
{
    tsamd::AtlasLayout lay;
    std::string err;
    const bool ok = tsamd::atlas_layout(n_triangles, texture_res, lay, err);
    if (cells_per_row_out) *cells_per_row_out = lay.cells_per_row;
    if (cell_out) *cell_out = lay.cell;
    if (leg_out) *leg_out = lay.leg;
    return ok ? TSAMD_OK : capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "atlas: " + err);
}

int tsamd_atlas_bake_positions(const float *v_pos_dev, int64_t n_vertices, const int32_t *tri_dev, int64_t n_triangles, int32_t texture_res,
                               float *positions_out_dev, int32_t *owner_out_dev, void *stream)
{
    tsamd::AtlasLayout lay;
    std::string err;
    if (!tsamd::atlas_layout(n_triangles, texture_res, lay, err)) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "atlas: " + err);
    if (n_vertices < 0) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "atlas: n_vertices < 0");
    if (!tri_dev || !positions_out_dev || !owner_out_dev || (n_vertices > 0 && !v_pos_dev))
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "atlas: v_pos_dev / tri_dev / positions_out_dev / owner_out_dev is null");
    TSAMD_HIP(tsamd::launch_atlas_bake_positions(v_pos_dev, n_vertices, tri_dev, n_triangles, texture_res, lay, positions_out_dev, owner_out_dev,
                                                 static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_texture(const float *tex_dev, int64_t tex_batch, int32_t tex_height, int32_t tex_width, int32_t n_channels, const float *uv_dev,
                  int64_t batch, int32_t height, int32_t width, int32_t filter_mode, int32_t boundary_mode, float *out_dev, void *stream)
{
    const int rc = check_texture(tex_batch, tex_height, tex_width, n_channels, batch, height, width, filter_mode, boundary_mode);
    if (rc) return rc;
    const int64_t per_image = int64_t(height) * width, pixels = batch * per_image;
    if (pixels > 0 && (!tex_dev || !uv_dev || !out_dev)) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "texture: tex_dev / uv_dev / out_dev is null");
    if (reinterpret_cast<uintptr_t>(uv_dev) % 8) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "texture: uv_dev is not aligned to 8 bytes");
    TSAMD_HIP(tsamd::launch_texture(tex_dev, tex_batch, tex_height, tex_width, n_channels, uv_dev, pixels, per_image, filter_mode, boundary_mode,
                                    out_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_texture_backward(const float *tex_dev, int64_t tex_batch, int32_t tex_height, int32_t tex_width, int32_t n_channels,
                           const float *uv_dev, int64_t batch, int32_t height, int32_t width, int32_t filter_mode, int32_t boundary_mode,
                           const float *grad_out_dev, float *grad_tex_dev, float *grad_uv_dev, void *stream)
{
    const int rc = check_texture(tex_batch, tex_height, tex_width, n_channels, batch, height, width, filter_mode, boundary_mode);
    if (rc) return rc;
    if (grad_uv_dev && filter_mode != TSAMD_TEX_FILTER_LINEAR)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "texture: grad_uv_dev is offered for TSAMD_TEX_FILTER_LINEAR only (nearest has no uv gradient)");
    const int64_t per_image = int64_t(height) * width, pixels = batch * per_image;
    if (pixels > 0 && (!uv_dev || !grad_out_dev)) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "texture: uv_dev / grad_out_dev is null");
    if (pixels > 0 && grad_uv_dev && !tex_dev) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "texture: tex_dev is null (grad_uv_dev needs it)");
    if (reinterpret_cast<uintptr_t>(uv_dev) % 8 || reinterpret_cast<uintptr_t>(grad_uv_dev) % 8)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "texture: uv_dev / grad_uv_dev is not aligned to 8 bytes");
    TSAMD_HIP(tsamd::launch_texture_backward(tex_dev, tex_batch, tex_height, tex_width, n_channels, uv_dev, pixels, per_image, filter_mode,
                                             boundary_mode, grad_out_dev, grad_tex_dev, grad_uv_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

}  // extern "C"
