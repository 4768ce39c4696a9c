// C ABI of the mesh voxeliser (include/tssplat_amd.h, tsamd_voxel_workspace_bytes / _winding / _occupancy): stateless entry points over
// caller-owned buffers.  Every argument is checked before the first device call.
#include "capi_common.h"
#include "voxel.h"

using tsamd::capi_fail;
using tsamd::check_buffers;

namespace {

// everything the two calls share: the sizes, the grid, the workspace and the stats, the mesh pointers
int check_common(const float *v_dev, int64_t n_vertices, const int32_t *faces_dev, int64_t n_triangles, int32_t grid, double lo, double hi, const void *workspace_dev,
                 const void *stats_out_dev)
{
    int rc = tsamd::check_vertex_count(n_vertices, "faces");
    if (rc) return rc;
    if (n_triangles < 0 || n_triangles > INT32_MAX) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "n_triangles out of range (0 .. 2^31 - 1)");
    if ((rc = tsamd::check_grid(grid, tsamd::kVoxelMinGrid, tsamd::kVoxelMaxGrid)) || (rc = tsamd::check_cube(lo, hi, grid, "grid"))) return rc;
    if ((rc = check_buffers({{workspace_dev, "workspace_dev", 8}, {stats_out_dev, "stats_out_dev", 8}}))) return rc;
    if (n_triangles > 0 && (rc = check_buffers({{faces_dev, "faces_dev", 4}}))) return rc;
    if (n_triangles > 0 && n_vertices > 0 && (rc = check_buffers({{v_dev, "v_dev", 4}}))) return rc;
    return TSAMD_OK;
}

}  // namespace

extern "C" {

int64_t tsamd_voxel_workspace_bytes(int32_t grid)
{
    return grid >= tsamd::kVoxelMinGrid && grid <= tsamd::kVoxelMaxGrid ? tsamd::voxel_workspace_bytes(grid, 3) : -1;
}

int tsamd_voxel_winding(const float *v_dev, int64_t n_vertices, const int32_t *faces_dev, int64_t n_triangles, int32_t grid, double lo, double hi, int32_t axis,
                        void *workspace_dev, int32_t *w_out_dev, int64_t *stats_out_dev, void *stream)
{
    int rc = check_common(v_dev, n_vertices, faces_dev, n_triangles, grid, lo, hi, workspace_dev, stats_out_dev);
    if (rc) return rc;
    if (axis < 0 || axis > 2) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "axis must be 0, 1 or 2");
    if ((rc = check_buffers({{w_out_dev, "w_out_dev", 4}}))) return rc;
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
    if ((rc = check_buffers({{occ_out_dev, "occ_out_dev", 1}}))) return rc;
    TSAMD_HIP(tsamd::launch_voxel_occupancy(v_dev, n_vertices, faces_dev, n_triangles, grid, lo, hi, rule, rays, workspace_dev, occ_out_dev,
                                            stats_out_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

}  // extern "C"
