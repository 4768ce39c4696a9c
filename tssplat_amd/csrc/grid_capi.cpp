// C ABI of the hash-grid encoding (include/tssplat_amd.h, "hash-grid encoding" section): the host-side level layout and the
// stateless forward / backward entry points.  The caller owns every buffer and names the device by making it current.
#include <cmath>
#include <cstdint>
#include <string>

#include "capi_common.h"
#include "grid.h"

using tsamd::capi_fail;

namespace tsamd {

bool grid_layout(int32_t n_levels, int32_t n_features, int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale,
                 int32_t dense, GridLevels &lv, int64_t &n_params, std::string &err)
{
    if (n_levels < 1 || n_levels > kGridMaxLevels) {
        err = "n_levels must be 1 .. " + std::to_string(kGridMaxLevels);
        return false;
    }
    if (n_features != 1 && n_features != 2 && n_features != 4 && n_features != 8) {
        err = "n_features_per_level must be 1, 2, 4 or 8";
        return false;
    }
    if (log2_hashmap_size < 1 || log2_hashmap_size > 30) {
        err = "log2_hashmap_size must be 1 .. 30";
        return false;
    }
    if (base_resolution < 1 || !(per_level_scale >= 1.0f) || !std::isfinite(per_level_scale)) {
        err = "base_resolution must be >= 1 and per_level_scale a finite value >= 1";
        return false;
    }
    if (dense != 0 && dense != 1) {
        err = "dense must be 0 (Hash) or 1 (Dense)";
        return false;
    }
    const uint64_t T = uint64_t(1) << log2_hashmap_size;
    // tiny-cuda-nn grid_scale / grid_resolution, in float32 and in this order; log2f / exp2f correctly rounded (evaluated in
    // double and rounded once), so that the grid does not depend on the libm (tests/hashgrid_oracle.py does the same)
    const float log2_scale = float(std::log2(double(per_level_scale)));
    int64_t offset = 0;
    lv = GridLevels{};
    lv.n_levels = n_levels;
    for (int l = 0; l < n_levels; ++l) {
        const float scale = float(std::exp2(double(float(l) * log2_scale))) * float(base_resolution) - 1.0f;
        if (!(scale >= 0.0f) || scale > 65535.0f) {
            err = "level " + std::to_string(l) + ": grid scale out of range (resolution above 65536)";
            return false;
        }
        const uint32_t res = uint32_t(std::ceil(scale)) + 1;
        const uint64_t cube = uint64_t(res) * res * res;
        uint64_t entries = (cube + 7) / 8 * 8;
        if (!dense && entries > T) entries = T;
        if (entries > 0xffffffffull / uint64_t(n_features)) {
            err = "level " + std::to_string(l) + ": more than 2^32 parameters in one level (a dense grid this fine is not offered)";
            return false;
        }
        // grid_index: the stride loop runs in uint32 while the stride stays <= entries; hashed when it passed them
        uint32_t stride = 1;
        for (int d = 0; d < 3 && stride <= entries; ++d) stride *= res;
        lv.offset[l] = offset;
        lv.entries[l] = uint32_t(entries);
        lv.res[l] = res;
        lv.scale[l] = scale;
        lv.hashed[l] = (!dense && entries < stride) ? 1u : 0u;
        offset += int64_t(entries);
    }
    n_params = offset * n_features;
    return true;
}

}  // namespace tsamd

namespace {

int layout_or_fail(int32_t n_levels, int32_t n_features, int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale,
                   int32_t dense, tsamd::GridLevels &lv, int64_t &n_params)
{
    std::string err;
    if (!tsamd::grid_layout(n_levels, n_features, log2_hashmap_size, base_resolution, per_level_scale, dense, lv, n_params, err))
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: " + err);
    // the coarse levels whose table fits in LDS (a prefix: entries never decrease with the level)
    lv.lds_levels = 0;
    while (lv.lds_levels < n_levels && int64_t(lv.entries[lv.lds_levels]) * n_features * 4 <= tsamd::kGridLdsBytes) ++lv.lds_levels;
    return TSAMD_OK;
}

int check_pointers(int64_t n_points, const float *x_dev, const float *params_dev, int32_t n_features)
{
    if (n_points < 0) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: n_points < 0");
    if (n_points > (int64_t(1) << 40)) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: n_points above 2^40");
    if (!params_dev) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: params_dev is null");
    if (n_points > 0 && !x_dev) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: x_dev is null");
    // one vector load / store per entry: float2 for F = 2, float4 for F >= 4
    const uintptr_t align = n_features == 1 ? 4 : (n_features == 2 ? 8 : 16);
    if (reinterpret_cast<uintptr_t>(params_dev) % align)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: params_dev is not aligned to n_features_per_level floats (max 16 B)");
    if (reinterpret_cast<uintptr_t>(x_dev) % 4) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: x_dev is not float-aligned");
    return TSAMD_OK;
}

}  // namespace

extern "C" {

int tsamd_grid_layout(int32_t n_levels, int32_t n_features_per_level, int32_t log2_hashmap_size, int32_t base_resolution,
                      float per_level_scale, int32_t dense, int64_t *offsets_out, int32_t *resolution_out, int32_t *hashed_out,
                      float *scale_out, int64_t *n_params_out)
{
    tsamd::GridLevels lv;
    int64_t n_params = 0;
    const int rc = layout_or_fail(n_levels, n_features_per_level, log2_hashmap_size, base_resolution, per_level_scale, dense, lv, n_params);
    if (rc) return rc;
    for (int l = 0; l < n_levels; ++l) {
        if (offsets_out) offsets_out[l] = lv.offset[l];
        if (resolution_out) resolution_out[l] = int32_t(lv.res[l]);
        if (hashed_out) hashed_out[l] = int32_t(lv.hashed[l]);
        if (scale_out) scale_out[l] = lv.scale[l];
    }
    if (offsets_out) offsets_out[n_levels] = n_params / n_features_per_level;
    if (n_params_out) *n_params_out = n_params;
    return TSAMD_OK;
}

int tsamd_grid_encode(const float *x_dev, int64_t n_points, const float *params_dev, int32_t n_levels, int32_t n_features_per_level,
                      int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale, int32_t dense, float *out_dev, void *stream)
{
    tsamd::GridLevels lv;
    int64_t n_params = 0;
    int rc = layout_or_fail(n_levels, n_features_per_level, log2_hashmap_size, base_resolution, per_level_scale, dense, lv, n_params);
    if (rc) return rc;
    rc = check_pointers(n_points, x_dev, params_dev, n_features_per_level);
    if (rc) return rc;
    if (n_points > 0 && !out_dev) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: out_dev is null");
    if (reinterpret_cast<uintptr_t>(out_dev) % (n_features_per_level == 1 ? 4 : (n_features_per_level == 2 ? 8 : 16)))
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: out_dev is not aligned to n_features_per_level floats (max 16 B)");
    TSAMD_HIP(tsamd::launch_grid_encode(x_dev, n_points, params_dev, lv, n_features_per_level, out_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_grid_encode_backward(const float *x_dev, int64_t n_points, const float *params_dev, int32_t n_levels, int32_t n_features_per_level,
                               int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale, int32_t dense,
                               const float *grad_out_dev, float *grad_params_dev, float *grad_x_dev, void *stream)
{
    tsamd::GridLevels lv;
    int64_t n_params = 0;
    int rc = layout_or_fail(n_levels, n_features_per_level, log2_hashmap_size, base_resolution, per_level_scale, dense, lv, n_params);
    if (rc) return rc;
    rc = check_pointers(n_points, x_dev, params_dev, n_features_per_level);
    if (rc) return rc;
    if (n_points > 0 && !grad_out_dev) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: grad_out_dev is null");
    const uintptr_t align = n_features_per_level == 1 ? 4 : (n_features_per_level == 2 ? 8 : 16);
    if (reinterpret_cast<uintptr_t>(grad_out_dev) % align || reinterpret_cast<uintptr_t>(grad_params_dev) % align)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: grad_out_dev / grad_params_dev not aligned to n_features_per_level floats (max 16 B)");
    if (reinterpret_cast<uintptr_t>(grad_x_dev) % 4) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: grad_x_dev is not float-aligned");
    TSAMD_HIP(tsamd::launch_grid_encode_backward(x_dev, n_points, params_dev, lv, n_features_per_level, grad_out_dev, grad_params_dev, grad_x_dev,
                                                 static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int64_t tsamd_grid_sorted_chunk_points(void) { return tsamd::kGridSortedChunk; }

int tsamd_grid_backward_sorted_workspace_bytes(int64_t n_points, int32_t n_levels, int32_t n_features_per_level, int32_t log2_hashmap_size,
                                               int32_t base_resolution, float per_level_scale, int32_t dense, int64_t *bytes_out)
{
    tsamd::GridLevels lv;
    int64_t n_params = 0;
    const int rc = layout_or_fail(n_levels, n_features_per_level, log2_hashmap_size, base_resolution, per_level_scale, dense, lv, n_params);
    if (rc) return rc;
    if (n_points < 0) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: n_points < 0");
    if (!bytes_out) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: bytes_out is null");
    *bytes_out = tsamd::grid_sorted_workspace(n_points, n_features_per_level).bytes;
    return TSAMD_OK;
}

int tsamd_grid_encode_backward_sorted(const float *x_dev, int64_t n_points, const float *params_dev, int32_t n_levels,
                                      int32_t n_features_per_level, int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale,
                                      int32_t dense, const float *grad_out_dev, float *grad_params_dev, float *grad_x_dev, void *workspace_dev,
                                      int64_t workspace_bytes, void *stream)
{
    tsamd::GridLevels lv;
    int64_t n_params = 0;
    int rc = layout_or_fail(n_levels, n_features_per_level, log2_hashmap_size, base_resolution, per_level_scale, dense, lv, n_params);
    if (rc) return rc;
    rc = check_pointers(n_points, x_dev, params_dev, n_features_per_level);
    if (rc) return rc;
    if (n_points > 0 && !grad_out_dev) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: grad_out_dev is null");
    const uintptr_t align = n_features_per_level == 1 ? 4 : (n_features_per_level == 2 ? 8 : 16);
    if (reinterpret_cast<uintptr_t>(grad_out_dev) % align || reinterpret_cast<uintptr_t>(grad_params_dev) % align)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: grad_out_dev / grad_params_dev not aligned to n_features_per_level floats (max 16 B)");
    if (reinterpret_cast<uintptr_t>(grad_x_dev) % 4) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: grad_x_dev is not float-aligned");
    if (grad_params_dev) {                            // (dL/dx only needs no workspace)
        const int64_t need = tsamd::grid_sorted_workspace(n_points, n_features_per_level).bytes;
        if (need > 0 && !workspace_dev) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: workspace_dev is null");
        if (reinterpret_cast<uintptr_t>(workspace_dev) % tsamd::kGridWorkspaceAlign)
            return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: workspace_dev is not aligned to 256 bytes");
        if (workspace_bytes < need)
            return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: workspace_bytes = " + std::to_string(workspace_bytes) + ", the sorted backward needs " +
                                                             std::to_string(need) + " (tsamd_grid_backward_sorted_workspace_bytes)");
    }
    TSAMD_HIP(tsamd::launch_grid_encode_backward_sorted(x_dev, n_points, params_dev, lv, n_features_per_level, grad_out_dev, grad_params_dev,
                                                        grad_x_dev, workspace_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_grid_plan_bytes(int64_t n_points, int32_t n_levels, int32_t n_features_per_level, int32_t log2_hashmap_size, int32_t base_resolution,
                          float per_level_scale, int32_t dense, int64_t *bytes_out)
{
    tsamd::GridLevels lv;
    int64_t n_params = 0;
    const int rc = layout_or_fail(n_levels, n_features_per_level, log2_hashmap_size, base_resolution, per_level_scale, dense, lv, n_params);
    if (rc) return rc;
    if (n_points < 0) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: n_points < 0");
    if (n_points > (int64_t(1) << 40)) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: n_points above 2^40");
    if (!bytes_out) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: bytes_out is null");
    *bytes_out = tsamd::grid_plan_bytes(n_points, n_levels);
    return TSAMD_OK;
}

int tsamd_grid_backward_planned_workspace_bytes(int64_t n_points, int32_t n_levels, int32_t n_features_per_level, int32_t log2_hashmap_size,
                                                int32_t base_resolution, float per_level_scale, int32_t dense, int64_t *bytes_out)
{
    tsamd::GridLevels lv;
    int64_t n_params = 0;
    const int rc = layout_or_fail(n_levels, n_features_per_level, log2_hashmap_size, base_resolution, per_level_scale, dense, lv, n_params);
    if (rc) return rc;
    if (n_points < 0) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: n_points < 0");
    if (!bytes_out) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: bytes_out is null");
    *bytes_out = tsamd::grid_planned_workspace(n_points, n_features_per_level, n_levels).bytes;
    return TSAMD_OK;
}

namespace {

// The plan's and a workspace's checks, shared by the plan build and the planned backward.
int check_plan_buffers(int64_t n_points, int32_t n_levels, const void *plan_dev, int64_t plan_bytes, const void *workspace_dev,
                       int64_t workspace_bytes, int64_t workspace_need, const char *workspace_query)
{
    const int64_t plan_need = tsamd::grid_plan_bytes(n_points, n_levels);
    if (plan_need > 0 && !plan_dev) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: plan_dev is null");
    if (reinterpret_cast<uintptr_t>(plan_dev) % tsamd::kGridWorkspaceAlign)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: plan_dev is not aligned to 256 bytes");
    if (plan_bytes < plan_need)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: plan_bytes = " + std::to_string(plan_bytes) + ", the plan needs " +
                                                         std::to_string(plan_need) + " (tsamd_grid_plan_bytes)");
    if (workspace_need > 0 && !workspace_dev) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: workspace_dev is null");
    if (reinterpret_cast<uintptr_t>(workspace_dev) % tsamd::kGridWorkspaceAlign)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: workspace_dev is not aligned to 256 bytes");
    if (workspace_bytes < workspace_need)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: workspace_bytes = " + std::to_string(workspace_bytes) + ", needed: " +
                                                         std::to_string(workspace_need) + " (" + workspace_query + ")");
    return TSAMD_OK;
}

}  // namespace

int tsamd_grid_plan_build(const float *x_dev, int64_t n_points, int32_t n_levels, int32_t n_features_per_level, int32_t log2_hashmap_size,
                          int32_t base_resolution, float per_level_scale, int32_t dense, void *plan_dev, int64_t plan_bytes, void *workspace_dev,
                          int64_t workspace_bytes, void *stream)
{
    tsamd::GridLevels lv;
    int64_t n_params = 0;
    int rc = layout_or_fail(n_levels, n_features_per_level, log2_hashmap_size, base_resolution, per_level_scale, dense, lv, n_params);
    if (rc) return rc;
    if (n_points < 0) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: n_points < 0");
    if (n_points > (int64_t(1) << 40)) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: n_points above 2^40");
    if (n_points > 0 && !x_dev) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: x_dev is null");
    if (reinterpret_cast<uintptr_t>(x_dev) % 4) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: x_dev is not float-aligned");
    rc = check_plan_buffers(n_points, n_levels, plan_dev, plan_bytes, workspace_dev, workspace_bytes,
                            tsamd::grid_sorted_workspace(n_points, n_features_per_level).bytes, "tsamd_grid_backward_sorted_workspace_bytes");
    if (rc) return rc;
    TSAMD_HIP(tsamd::launch_grid_plan_build(x_dev, n_points, lv, n_features_per_level, plan_dev, workspace_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_grid_encode_backward_planned(const float *x_dev, int64_t n_points, int32_t n_levels, int32_t n_features_per_level,
                                       int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale, int32_t dense,
                                       const float *grad_out_dev, float *grad_params_dev, const void *plan_dev, int64_t plan_bytes,
                                       void *workspace_dev, int64_t workspace_bytes, void *stream)
{
    tsamd::GridLevels lv;
    int64_t n_params = 0;
    int rc = layout_or_fail(n_levels, n_features_per_level, log2_hashmap_size, base_resolution, per_level_scale, dense, lv, n_params);
    if (rc) return rc;
    if (n_points < 0) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: n_points < 0");
    if (n_points > (int64_t(1) << 40)) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: n_points above 2^40");
    if (n_points > 0 && !x_dev) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: x_dev is null");
    if (reinterpret_cast<uintptr_t>(x_dev) % 4) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: x_dev is not float-aligned");
    if (n_points > 0 && !grad_out_dev) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: grad_out_dev is null");
    if (n_points > 0 && !grad_params_dev) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: grad_params_dev is null");
    const uintptr_t align = n_features_per_level == 1 ? 4 : (n_features_per_level == 2 ? 8 : 16);
    if (reinterpret_cast<uintptr_t>(grad_out_dev) % align || reinterpret_cast<uintptr_t>(grad_params_dev) % align)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: grad_out_dev / grad_params_dev not aligned to n_features_per_level floats (max 16 B)");
    rc = check_plan_buffers(n_points, n_levels, plan_dev, plan_bytes, workspace_dev, workspace_bytes,
                            tsamd::grid_planned_workspace(n_points, n_features_per_level, n_levels).bytes,
                            "tsamd_grid_backward_planned_workspace_bytes");
    if (rc) return rc;
    TSAMD_HIP(tsamd::launch_grid_encode_backward_planned(x_dev, n_points, lv, n_features_per_level, grad_out_dev, grad_params_dev, plan_dev,
                                                         workspace_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

}  // extern "C"
