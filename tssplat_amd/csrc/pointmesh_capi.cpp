// C ABI of the exact point-to-triangle search (include/tssplat_amd.h, tsamd_nearest_on_mesh and its two queries): stateless entry
// points over caller-owned buffers.  Every argument is checked before the first device call.
#include "capi_common.h"
#include "pointmesh.h"

using tsamd::capi_fail;
using tsamd::check_buffers;

namespace {

int check_counts(int64_t n, int64_t n_triangles, int64_t least_triangles)
{
    if (n < 0 || n > INT32_MAX) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "n out of range (0 .. 2^31 - 1)");
    if (n_triangles < least_triangles || n_triangles > INT32_MAX)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, least_triangles ? "n_triangles out of range (1 .. 2^31 - 1: a query needs a triangle)"
                                                                     : "n_triangles out of range (0 .. 2^31 - 1)");
    return TSAMD_OK;
}

}  // namespace

extern "C" {

int64_t tsamd_nearest_on_mesh_workspace_bytes(int64_t n, int64_t n_triangles)
{
    if (n < 0 || n > INT32_MAX || n_triangles < 0 || n_triangles > INT32_MAX) return -1;
    return tsamd::pointmesh_workspace(n, n_triangles).bytes;
}

int tsamd_nearest_on_mesh_info(int64_t n, int64_t n_triangles, int32_t *block_out, int32_t *queries_per_lane_out, int32_t *tri_tile_out, int32_t *auto_chunks_out)
{
    int rc = check_counts(n, n_triangles, 0);
    if (rc) return rc;
    rc = tsamd::check_not_null({{block_out, "block_out"}, {queries_per_lane_out, "queries_per_lane_out"}, {tri_tile_out, "tri_tile_out"},
                                {auto_chunks_out, "auto_chunks_out"}});
    if (rc) return rc;
    *block_out = tsamd::kPointMeshBlock;
    *queries_per_lane_out = tsamd::kPointMeshQueriesPerLane;
    *tri_tile_out = tsamd::kPointMeshTile;
    *auto_chunks_out = tsamd::pointmesh_auto_chunks(n, n_triangles);
    return TSAMD_OK;
}

int tsamd_nearest_on_mesh(const float *query_dev, int64_t n, const float *v_dev, int64_t n_vertices, const int32_t *faces_dev, int64_t n_triangles,
                          int32_t ref_chunks, void *workspace_dev, float *d2_out_dev, int32_t *tri_out_dev, float *point_out_dev, void *stream)
{
    int rc = check_counts(n, n_triangles, 1);
    if (rc) return rc;
    if ((rc = tsamd::check_vertex_count(n_vertices, "faces"))) return rc;
    if (ref_chunks < 0 || ref_chunks > n_triangles || ref_chunks > tsamd::kPointMeshMaxChunks)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "ref_chunks out of range (0 = automatic, else 1 .. min(n_triangles, 65535))");
    if (n == 0) return TSAMD_OK;                                           // nothing to write
    if ((rc = check_buffers({{query_dev, "query_dev", 4}, {faces_dev, "faces_dev", 4}, {workspace_dev, "workspace_dev", 16}, {d2_out_dev, "d2_out_dev", 4},
                             {tri_out_dev, "tri_out_dev", 4}})))
        return rc;
    if (n_vertices > 0 && (rc = check_buffers({{v_dev, "v_dev", 4}}))) return rc;
    if (point_out_dev && (rc = tsamd::check_aligned(point_out_dev, "point_out_dev", 4))) return rc;
    const int32_t chunks = ref_chunks ? ref_chunks : tsamd::pointmesh_auto_chunks(n, n_triangles);
    TSAMD_HIP(tsamd::launch_nearest_on_mesh(query_dev, n, v_dev, n_vertices, faces_dev, n_triangles, chunks, workspace_dev, d2_out_dev, tri_out_dev,
                                            point_out_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

}  // extern "C"
