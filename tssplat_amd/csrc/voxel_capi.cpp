// C ABI of the mesh voxeliser (include/tssplat_amd.h, tsamd_voxel_workspace_bytes / _winding / _occupancy): stateless entry points over
// caller-owned buffers.  Every argument is checked before the first device call.
#include <cmath>

#include "capi_common.h"
#include "voxel.h"

using tsamd::capi_fail;
using tsamd::check_not_null;

namespace {

int check_aligned(const void *ptr, const char *name, uintptr_t bytes)
{
    if (reinterpret_cast<uintptr_t>(ptr) % bytes != 0)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, std::string(name) + " must be " + std::to_string(bytes) + "-byte aligned");
    return TSAMD_OK;
}

bool grid_ok(int32_t grid) { return grid >= tsamd::kVoxelMinGrid && grid <= tsamd::kVoxelMaxGrid; }

// everything the two calls share: the sizes, the grid, the mesh pointers, the workspace and the stats
int check_common(const float *v_dev, int64_t n_vertices, const int32_t *faces_dev, int64_t n_triangles, int32_t grid, double lo, double hi, const void *workspace_dev,
                 const void *stats_out_dev)
{
    if (n_vertices < 0 || n_vertices > INT32_MAX) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "n_vertices out of range (0 .. 2^31 - 1: faces holds 32-bit indices)");
    if (n_triangles < 0 || n_triangles > INT32_MAX) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "n_triangles out of range (0 .. 2^31 - 1)");
    if (!grid_ok(grid)) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "grid out of range (1 .. 512)");
    if (!(std::isfinite(lo) && std::isfinite(hi) && lo < hi && std::isfinite(hi - lo) && (hi - lo) / double(grid) > 0.0))
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "lo / hi must be finite with lo < hi and (hi - lo) / grid > 0");
    int rc;
    if ((rc = check_not_null({{workspace_dev, "workspace_dev"}, {stats_out_dev, "stats_out_dev"}})) || (rc = check_aligned(workspace_dev, "workspace_dev", 8)) ||
        (rc = check_aligned(stats_out_dev, "stats_out_dev", 8)))
        return rc;
    if (n_triangles > 0 && ((rc = check_not_null({{faces_dev, "faces_dev"}})) || (rc = check_aligned(faces_dev, "faces_dev", 4)))) return rc;
    if (n_triangles > 0 && n_vertices > 0 && ((rc = check_not_null({{v_dev, "v_dev"}})) || (rc = check_aligned(v_dev, "v_dev", 4)))) return rc;
    return TSAMD_OK;
}

}  // namespace

extern "C" {

int64_t tsamd_voxel_workspace_bytes(int32_t grid)
{
    return grid_ok(grid) ? tsamd::voxel_workspace_bytes(grid, 3) : -1;
}

int tsamd_voxel_winding(const float *v_dev, int64_t n_vertices, const int32_t *faces_dev, int64_t n_triangles, int32_t grid, double lo, double hi, int32_t axis,
                        void *workspace_dev, int32_t *w_out_dev, int64_t *stats_out_dev, void *stream)
{
    int rc = check_common(v_dev, n_vertices, faces_dev, n_triangles, grid, lo, hi, workspace_dev, stats_out_dev);
    if (rc) return rc;
    if (axis < 0 || axis > 2) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "axis must be 0, 1 or 2");
    if ((rc = check_not_null({{w_out_dev, "w_out_dev"}})) || (rc = check_aligned(w_out_dev, "w_out_dev", 4))) return rc;
    TSAMD_HIP(tsamd::launch_voxel_winding(v_dev, n_vertices, faces_dev, n_triangles, grid, lo, hi, axis, workspace_dev, w_out_dev,
                                          stats_out_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_voxel_occupancy(const float *v_dev, int64_t n_vertices, const int32_t *faces_dev, int64_t n_triangles, int32_t grid, double lo, double hi, int32_t rule,
                          int32_t rays, void *workspace_dev, uint8_t *occ_out_dev, int64_t *stats_out_dev, void *stream)
{
    int rc = check_common(v_dev, n_vertices, faces_dev, n_triangles, grid, lo, hi, workspace_dev, stats_out_dev);
    if (rc) return rc;
    if (rule != tsamd::kVoxelRuleNonzero && rule != tsamd::kVoxelRulePositive && rule != tsamd::kVoxelRuleOdd)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "rule must be TSAMD_VOXEL_NONZERO (0), TSAMD_VOXEL_POSITIVE (1) or TSAMD_VOXEL_ODD (2)");
    if (rays != 1 && rays != 3) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "rays must be 1 or 3");
    if ((rc = check_not_null({{occ_out_dev, "occ_out_dev"}}))) return rc;
    TSAMD_HIP(tsamd::launch_voxel_occupancy(v_dev, n_vertices, faces_dev, n_triangles, grid, lo, hi, rule, rays, workspace_dev, occ_out_dev,
                                            stats_out_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

}  // extern "C"
