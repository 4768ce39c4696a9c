// C ABI of the surface metrics (include/tssplat_amd.h, tsamd_sample_surface / tsamd_nearest_points and their two queries):
// stateless entry points over caller-owned buffers.  Every argument is checked before the first device call.
#include "capi_common.h"
#include "metrics.h"

using tsamd::capi_fail;
using tsamd::check_buffers;

extern "C" {

int64_t tsamd_nearest_points_workspace_bytes(int64_t n)
{
    if (n < 0 || n > INT32_MAX) return -1;
    return n * int64_t(sizeof(uint64_t));
}

int tsamd_nearest_points_info(int64_t n, int64_t m, int32_t *block_out, int32_t *queries_per_lane_out, int32_t *ref_tile_out, int32_t *auto_chunks_out)
{
    if (n < 0 || n > INT32_MAX) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "n out of range (0 .. 2^31 - 1)");
    if (m < 0 || m > INT32_MAX) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "m out of range (0 .. 2^31 - 1)");
    int rc = tsamd::check_not_null({{block_out, "block_out"}, {queries_per_lane_out, "queries_per_lane_out"}, {ref_tile_out, "ref_tile_out"},
                                    {auto_chunks_out, "auto_chunks_out"}});
    if (rc) return rc;
    *block_out = tsamd::kNearestBlock;
    *queries_per_lane_out = tsamd::kNearestQueriesPerLane;
    *ref_tile_out = tsamd::kNearestTile;
    *auto_chunks_out = tsamd::nearest_auto_chunks(n, m);
    return TSAMD_OK;
}

int tsamd_nearest_points(const float *query_dev, int64_t n, const float *ref_dev, int64_t m, int32_t ref_chunks, void *workspace_dev, float *d2_out_dev,
                         int32_t *idx_out_dev, void *stream)
{
    if (n < 0 || n > INT32_MAX) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "n out of range (0 .. 2^31 - 1)");
    if (m < 1 || m > INT32_MAX) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "m out of range (1 .. 2^31 - 1: a query needs a ref point)");
    if (ref_chunks < 0 || ref_chunks > m || ref_chunks > tsamd::kNearestMaxChunks)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "ref_chunks out of range (0 = automatic, else 1 .. min(m, 65535))");
    if (n == 0) return TSAMD_OK;                                           // nothing to write
    int rc = check_buffers({{query_dev, "query_dev", 4}, {ref_dev, "ref_dev", 4}, {workspace_dev, "workspace_dev", 8}, {d2_out_dev, "d2_out_dev", 4},
                            {idx_out_dev, "idx_out_dev", 4}});
    if (rc) return rc;
    const int32_t chunks = ref_chunks ? ref_chunks : tsamd::nearest_auto_chunks(n, m);
    TSAMD_HIP(tsamd::launch_nearest_points(query_dev, n, ref_dev, m, chunks, static_cast<uint64_t *>(workspace_dev), d2_out_dev, idx_out_dev,
                                           static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_sample_surface(int32_t phase, const float *v_dev, int64_t n_vertices, const int32_t *faces_dev, int64_t n_triangles, int64_t *prefix_dev,
                         void *workspace_dev, int64_t n_samples, uint64_t seed, float *points_out_dev, float *normals_out_dev, int32_t *tri_out_dev,
                         void *stream)
{
    if (phase != tsamd::kSampleWeights && phase != tsamd::kSampleDraw)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "phase must be TSAMD_SAMPLE_WEIGHTS (0) or TSAMD_SAMPLE_DRAW (1)");
    int rc = tsamd::check_vertex_count(n_vertices, "faces");
    if (rc) return rc;
    if (n_triangles < 1 || n_triangles > INT32_MAX) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "n_triangles out of range (1 .. 2^31 - 1)");
    if (n_samples < 0 || n_samples > INT32_MAX) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "n_samples out of range (0 .. 2^31 - 1)");
    if ((rc = check_buffers({{faces_dev, "faces_dev", 4}, {prefix_dev, "prefix_dev", 8}}))) return rc;
    if (n_vertices > 0 && (rc = check_buffers({{v_dev, "v_dev", 4}}))) return rc;
    if (phase == tsamd::kSampleWeights) {
        if ((rc = check_buffers({{workspace_dev, "workspace_dev", 8}}))) return rc;
        TSAMD_HIP(tsamd::launch_sample_weights(v_dev, n_vertices, faces_dev, n_triangles, prefix_dev, static_cast<uint64_t *>(workspace_dev),
                                               static_cast<hipStream_t>(stream)));
        return TSAMD_OK;
    }
    if (n_samples == 0) return TSAMD_OK;                                   // nothing to write
    if ((rc = check_buffers({{points_out_dev, "points_out_dev", 4}, {normals_out_dev, "normals_out_dev", 4}, {tri_out_dev, "tri_out_dev", 4}}))) return rc;
    TSAMD_HIP(tsamd::launch_sample_draw(v_dev, n_vertices, faces_dev, n_triangles, prefix_dev, n_samples, seed, points_out_dev, normals_out_dev, tri_out_dev,
                                        static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

}  // extern "C"
