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

int fail(const std::string &what) { return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid encoding: " + what); }

#define TSAMD_GRID_CHECK(check)                  \
    do {                                         \
        if (const int rc_ = (check)) return rc_; \
    } while (0)

// The config's level table, as the kernels take it.
int check_config(int32_t n_levels, int32_t n_features, int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale, int32_t dense,
                 tsamd::GridLevels &lv, int64_t *n_params_out = nullptr)
{
    std::string err;
    int64_t n_params = 0;
    if (!tsamd::grid_layout(n_levels, n_features, log2_hashmap_size, base_resolution, per_level_scale, dense, lv, n_params, err)) return fail(err);
    // the coarse levels whose table fits in LDS (a prefix: entries never decrease with the level)
    lv.lds_levels = 0;
    while (lv.lds_levels < n_levels && int64_t(lv.entries[lv.lds_levels]) * n_features * 4 <= tsamd::kGridLdsBytes) ++lv.lds_levels;
    if (n_params_out) *n_params_out = n_params;
    return TSAMD_OK;
}

// `limited`: whether the entry point bounds n_points by 2^40.  The two workspace size queries (sorted and planned) never did
// and still do not (their answer is constant from one chunk on); every other entry point does.
int check_count(int64_t n_points, bool limited)
{
    if (n_points < 0) return fail("n_points < 0");
    if (limited && n_points > (int64_t(1) << 40)) return fail("n_points above 2^40");
    return TSAMD_OK;
}

int check_float_aligned(const void *p, const char *name)
{
    if (reinterpret_cast<uintptr_t>(p) % 4) return fail(std::string(name) + " is not float-aligned");
    return TSAMD_OK;
}

int check_points(int64_t n_points, const float *x_dev)
{
    TSAMD_GRID_CHECK(check_count(n_points, true));
    if (n_points > 0 && !x_dev) return fail("x_dev is null");
    return check_float_aligned(x_dev, "x_dev");
}

// A size query's own arguments (`limited`: check_count).
int check_query(int64_t n_points, bool limited, const int64_t *bytes_out)
{
    TSAMD_GRID_CHECK(check_count(n_points, limited));
    return bytes_out ? TSAMD_OK : fail("bytes_out is null");
}

// One vector load / store per entry: float2 for F = 2, float4 for F >= 4.
int check_feature_aligned(const void *p, const char *name, int32_t n_features)
{
    const uintptr_t align = n_features == 1 ? 4 : (n_features == 2 ? 8 : 16);
    if (reinterpret_cast<uintptr_t>(p) % align) return fail(std::string(name) + " is not aligned to n_features_per_level floats (max 16 B)");
    return TSAMD_OK;
}

// A caller-owned device buffer `<name>_dev` of `<name>_bytes` bytes, sized by the query function `query`.
int check_buffer(const char *name, const void *p, int64_t bytes, int64_t need, const char *query)
{
    if (need > 0 && !p) return fail(std::string(name) + "_dev is null");
    if (reinterpret_cast<uintptr_t>(p) % tsamd::kGridWorkspaceAlign) return fail(std::string(name) + "_dev is not aligned to 256 bytes");
    if (bytes < need) return fail(std::string(name) + "_bytes = " + std::to_string(bytes) + ", needed: " + std::to_string(need) + " (" + query + ")");
    return TSAMD_OK;
}

// The points and the table, as the forward and the two backwards that differentiate through x take them.
int check_inputs(int64_t n_points, const float *x_dev, const float *params_dev, int32_t n_features)
{
    TSAMD_GRID_CHECK(check_points(n_points, x_dev));
    if (!params_dev) return fail("params_dev is null");
    return check_feature_aligned(params_dev, "params_dev", n_features);
}

// grad_out and the two gradients of the atomic and the sorted backward.
int check_gradients(int64_t n_points, const float *grad_out_dev, const float *grad_params_dev, const float *grad_x_dev, int32_t n_features)
{
    if (n_points > 0 && !grad_out_dev) return fail("grad_out_dev is null");
    TSAMD_GRID_CHECK(check_feature_aligned(grad_out_dev, "grad_out_dev", n_features));
    TSAMD_GRID_CHECK(check_feature_aligned(grad_params_dev, "grad_params_dev", n_features));
    return check_float_aligned(grad_x_dev, "grad_x_dev");
}

}  // namespace

extern "C" {

int tsamd_grid_layout(int32_t n_levels, int32_t n_features_per_level, int32_t log2_hashmap_size, int32_t base_resolution,
                      float per_level_scale, int32_t dense, int64_t *offsets_out, int32_t *resolution_out, int32_t *hashed_out,
                      float *scale_out, int64_t *n_params_out)
{
    tsamd::GridLevels lv;
    int64_t n_params = 0;
    TSAMD_GRID_CHECK(check_config(n_levels, n_features_per_level, log2_hashmap_size, base_resolution, per_level_scale, dense, lv, &n_params));
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
    TSAMD_GRID_CHECK(check_config(n_levels, n_features_per_level, log2_hashmap_size, base_resolution, per_level_scale, dense, lv));
    TSAMD_GRID_CHECK(check_inputs(n_points, x_dev, params_dev, n_features_per_level));
    if (n_points > 0 && !out_dev) return fail("out_dev is null");
    TSAMD_GRID_CHECK(check_feature_aligned(out_dev, "out_dev", n_features_per_level));
    TSAMD_HIP(tsamd::launch_grid_encode(x_dev, n_points, params_dev, lv, n_features_per_level, out_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_grid_encode_backward(const float *x_dev, int64_t n_points, const float *params_dev, int32_t n_levels, int32_t n_features_per_level,
                               int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale, int32_t dense,
                               const float *grad_out_dev, float *grad_params_dev, float *grad_x_dev, void *stream)
{
    tsamd::GridLevels lv;
    TSAMD_GRID_CHECK(check_config(n_levels, n_features_per_level, log2_hashmap_size, base_resolution, per_level_scale, dense, lv));
    TSAMD_GRID_CHECK(check_inputs(n_points, x_dev, params_dev, n_features_per_level));
    TSAMD_GRID_CHECK(check_gradients(n_points, grad_out_dev, grad_params_dev, grad_x_dev, n_features_per_level));
    TSAMD_HIP(tsamd::launch_grid_encode_backward(x_dev, n_points, params_dev, lv, n_features_per_level, grad_out_dev, grad_params_dev, grad_x_dev,
                                                 static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int64_t tsamd_grid_sorted_chunk_points(void) { return tsamd::kGridSortedChunk; }

int tsamd_grid_backward_sorted_workspace_bytes(int64_t n_points, int32_t n_levels, int32_t n_features_per_level, int32_t log2_hashmap_size,
                                               int32_t base_resolution, float per_level_scale, int32_t dense, int64_t *bytes_out)
{
    tsamd::GridLevels lv;
    TSAMD_GRID_CHECK(check_config(n_levels, n_features_per_level, log2_hashmap_size, base_resolution, per_level_scale, dense, lv));
    TSAMD_GRID_CHECK(check_query(n_points, false, bytes_out));
    *bytes_out = tsamd::grid_sorted_workspace(n_points, n_features_per_level).bytes;
    return TSAMD_OK;
}

int tsamd_grid_encode_backward_sorted(const float *x_dev, int64_t n_points, const float *params_dev, int32_t n_levels,
                                      int32_t n_features_per_level, int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale,
                                      int32_t dense, const float *grad_out_dev, float *grad_params_dev, float *grad_x_dev, void *workspace_dev,
                                      int64_t workspace_bytes, void *stream)
{
    tsamd::GridLevels lv;
    TSAMD_GRID_CHECK(check_config(n_levels, n_features_per_level, log2_hashmap_size, base_resolution, per_level_scale, dense, lv));
    TSAMD_GRID_CHECK(check_inputs(n_points, x_dev, params_dev, n_features_per_level));
    TSAMD_GRID_CHECK(check_gradients(n_points, grad_out_dev, grad_params_dev, grad_x_dev, n_features_per_level));
    if (grad_params_dev)                              // (dL/dx only needs no workspace)
        TSAMD_GRID_CHECK(check_buffer("workspace", workspace_dev, workspace_bytes, tsamd::grid_sorted_workspace(n_points, n_features_per_level).bytes,
                                      "tsamd_grid_backward_sorted_workspace_bytes"));
    TSAMD_HIP(tsamd::launch_grid_encode_backward_sorted(x_dev, n_points, params_dev, lv, n_features_per_level, grad_out_dev, grad_params_dev,
                                                        grad_x_dev, workspace_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_grid_plan_bytes(int64_t n_points, int32_t n_levels, int32_t n_features_per_level, int32_t log2_hashmap_size, int32_t base_resolution,
                          float per_level_scale, int32_t dense, int64_t *bytes_out)
{
    tsamd::GridLevels lv;
    TSAMD_GRID_CHECK(check_config(n_levels, n_features_per_level, log2_hashmap_size, base_resolution, per_level_scale, dense, lv));
    TSAMD_GRID_CHECK(check_query(n_points, true, bytes_out));
    *bytes_out = tsamd::grid_plan_bytes(n_points, n_levels);
    return TSAMD_OK;
}

int tsamd_grid_backward_planned_workspace_bytes(int64_t n_points, int32_t n_levels, int32_t n_features_per_level, int32_t log2_hashmap_size,
                                                int32_t base_resolution, float per_level_scale, int32_t dense, int64_t *bytes_out)
{
    tsamd::GridLevels lv;
    TSAMD_GRID_CHECK(check_config(n_levels, n_features_per_level, log2_hashmap_size, base_resolution, per_level_scale, dense, lv));
    TSAMD_GRID_CHECK(check_query(n_points, false, bytes_out));
    *bytes_out = tsamd::grid_planned_workspace(n_points, n_features_per_level, n_levels).bytes;
    return TSAMD_OK;
}

int tsamd_grid_plan_build(const float *x_dev, int64_t n_points, int32_t n_levels, int32_t n_features_per_level, int32_t log2_hashmap_size,
                          int32_t base_resolution, float per_level_scale, int32_t dense, void *plan_dev, int64_t plan_bytes, void *workspace_dev,
                          int64_t workspace_bytes, void *stream)
{
    tsamd::GridLevels lv;
    TSAMD_GRID_CHECK(check_config(n_levels, n_features_per_level, log2_hashmap_size, base_resolution, per_level_scale, dense, lv));
    TSAMD_GRID_CHECK(check_points(n_points, x_dev));
    TSAMD_GRID_CHECK(check_buffer("plan", plan_dev, plan_bytes, tsamd::grid_plan_bytes(n_points, n_levels), "tsamd_grid_plan_bytes"));
    TSAMD_GRID_CHECK(check_buffer("workspace", workspace_dev, workspace_bytes, tsamd::grid_sorted_workspace(n_points, n_features_per_level).bytes,
                                  "tsamd_grid_backward_sorted_workspace_bytes"));
    TSAMD_HIP(tsamd::launch_grid_plan_build(x_dev, n_points, lv, n_features_per_level, plan_dev, workspace_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_grid_encode_backward_planned(const float *x_dev, int64_t n_points, int32_t n_levels, int32_t n_features_per_level,
                                       int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale, int32_t dense,
                                       const float *grad_out_dev, float *grad_params_dev, const void *plan_dev, int64_t plan_bytes,
                                       void *workspace_dev, int64_t workspace_bytes, void *stream)
{
    tsamd::GridLevels lv;
    TSAMD_GRID_CHECK(check_config(n_levels, n_features_per_level, log2_hashmap_size, base_resolution, per_level_scale, dense, lv));
    TSAMD_GRID_CHECK(check_points(n_points, x_dev));
    if (n_points > 0 && !grad_out_dev) return fail("grad_out_dev is null");
    if (n_points > 0 && !grad_params_dev) return fail("grad_params_dev is null");
    TSAMD_GRID_CHECK(check_feature_aligned(grad_out_dev, "grad_out_dev", n_features_per_level));
    TSAMD_GRID_CHECK(check_feature_aligned(grad_params_dev, "grad_params_dev", n_features_per_level));
    TSAMD_GRID_CHECK(check_buffer("plan", plan_dev, plan_bytes, tsamd::grid_plan_bytes(n_points, n_levels), "tsamd_grid_plan_bytes"));
    TSAMD_GRID_CHECK(check_buffer("workspace", workspace_dev, workspace_bytes,
                                  tsamd::grid_planned_workspace(n_points, n_features_per_level, n_levels).bytes,
                                  "tsamd_grid_backward_planned_workspace_bytes"));
    TSAMD_HIP(tsamd::launch_grid_encode_backward_planned(x_dev, n_points, lv, n_features_per_level, grad_out_dev, grad_params_dev, plan_dev,
                                                         workspace_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

}  // extern "C"
