// C ABI of the tet-sphere merge (include/tssplat_amd.h, tsamd_union_field / tsamd_surface_count / tsamd_surface_emit and the flood
// fill's tsamd_grid_components / tsamd_field_fill): stateless
// entry points over caller-owned buffers.  Every argument is checked before the first device call.
#include "capi_common.h"
#include "merge.h"

using tsamd::capi_fail;
using tsamd::check_cube;
using tsamd::check_grid;
using tsamd::check_level;
using tsamd::check_not_null;

extern "C" {

int tsamd_union_field(const float *tet_v_dev, int64_t n_vertices, const int32_t *elem_dev, int64_t n_tets, int32_t grid, double lo, double hi,
                      float *field_out_dev, void *stream)
{
    int rc = check_grid(grid, tsamd::kMergeMinGrid, tsamd::kMergeMaxGrid);
    if (rc || (rc = tsamd::check_vertex_count(n_vertices, "elem"))) return rc;
    if (n_tets < 0 || n_tets > tsamd::kMergeMaxTets) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "n_tets out of range (0 .. 2^30)");
    if ((rc = check_cube(lo, hi))) return rc;
    if (n_tets > 0 && (rc = check_not_null({{elem_dev, "elem_dev"}}))) return rc;
    if (n_tets > 0 && n_vertices > 0 && (rc = check_not_null({{tet_v_dev, "tet_v_dev"}}))) return rc;
    if ((rc = check_not_null({{field_out_dev, "field_out_dev"}}))) return rc;
    TSAMD_HIP(tsamd::launch_union_field(tet_v_dev, n_vertices, elem_dev, n_tets, grid, lo, (hi - lo) / grid, field_out_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_surface_count(const float *field_dev, int32_t grid, float level, uint8_t *vmask_out_dev, uint8_t *vcount_out_dev, uint8_t *tcount_out_dev,
                        int32_t *open_out_dev, void *stream)
{
    int rc = check_grid(grid, tsamd::kMergeMinGrid, tsamd::kMergeMaxGrid);
    if (rc || (rc = check_level(level))) return rc;
    if ((rc = check_not_null({{field_dev, "field_dev"}, {vmask_out_dev, "vmask_out_dev"}, {vcount_out_dev, "vcount_out_dev"}, {tcount_out_dev, "tcount_out_dev"},
                              {open_out_dev, "open_out_dev"}})))
        return rc;
    TSAMD_HIP(tsamd::launch_surface_count(field_dev, grid, level, vmask_out_dev, vcount_out_dev, tcount_out_dev, open_out_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_surface_emit(const float *field_dev, int32_t grid, double lo, double hi, float level, const uint8_t *vmask_dev, const int32_t *voffset_dev,
                       const int32_t *toffset_dev, int64_t n_vertices, int64_t n_triangles, float *v_out_dev, int32_t *faces_out_dev, void *stream)
{
    int rc = check_grid(grid, tsamd::kMergeMinGrid, tsamd::kMergeMaxGrid);
    if (rc || (rc = check_cube(lo, hi)) || (rc = check_level(level))) return rc;
    const int64_t nodes = int64_t(grid) * grid * grid;
    if (n_vertices < 0 || n_vertices > 7 * nodes) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "n_vertices out of range (0 .. 7 grid^3)");
    if (n_triangles < 0 || n_triangles > 12 * nodes) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "n_triangles out of range (0 .. 12 grid^3)");
    if ((rc = check_not_null({{field_dev, "field_dev"}, {vmask_dev, "vmask_dev"}, {voffset_dev, "voffset_dev"}, {toffset_dev, "toffset_dev"}}))) return rc;
    if (n_vertices > 0 && (rc = check_not_null({{v_out_dev, "v_out_dev"}}))) return rc;
    if (n_triangles > 0 && (rc = check_not_null({{faces_out_dev, "faces_out_dev"}}))) return rc;
    if (n_vertices == 0 && n_triangles == 0) return TSAMD_OK;             // nothing to write
    TSAMD_HIP(tsamd::launch_surface_emit(field_dev, grid, lo, (hi - lo) / grid, level, vmask_dev, voffset_dev, toffset_dev, n_vertices, n_triangles, v_out_dev,
                                         faces_out_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_grid_components(const float *field_dev, int32_t grid, float level, int32_t *label_out_dev, int32_t *status_out_dev, void *stream)
{
    int rc = check_grid(grid, tsamd::kMergeMinGrid, tsamd::kMergeMaxGrid);
    if (rc || (rc = check_level(level))) return rc;
    if ((rc = check_not_null({{field_dev, "field_dev"}, {label_out_dev, "label_out_dev"}, {status_out_dev, "status_out_dev"}}))) return rc;
    TSAMD_HIP(tsamd::launch_grid_components(field_dev, grid, level, label_out_dev, status_out_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_field_fill(const float *field_dev, int32_t grid, float level, int32_t mode, void *workspace_dev, float *field_out_dev, int32_t *stats_out_dev,
                     void *stream)
{
    int rc = check_grid(grid, tsamd::kMergeMinGrid, tsamd::kMergeMaxGrid);
    if (rc || (rc = check_level(level))) return rc;
    if (mode != tsamd::kFillCavities && mode != tsamd::kFillOuter)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "mode must be TSAMD_FILL_CAVITIES (1) or TSAMD_FILL_OUTER (2)");
    if ((rc = check_not_null({{field_dev, "field_dev"}, {workspace_dev, "workspace_dev"}, {field_out_dev, "field_out_dev"}, {stats_out_dev, "stats_out_dev"}})))
        return rc;
    if (field_out_dev == field_dev) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "field_out_dev must not be field_dev (the input is never modified)");
    if ((rc = tsamd::check_aligned(workspace_dev, "workspace_dev", 8))) return rc;
    TSAMD_HIP(tsamd::launch_field_fill(field_dev, grid, level, mode, static_cast<int32_t *>(workspace_dev), field_out_dev, stats_out_dev,
                                       static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

}  // extern "C"
