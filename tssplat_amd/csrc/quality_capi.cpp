// C ABI of the mesh-quality stage (include/tssplat_amd.h, tsamd_quality_*): stateless entry points over caller-owned buffers.
// Every argument is checked before the first device call.
#include "capi_common.h"
#include "quality.h"

using tsamd::capi_fail;
using tsamd::check_buffers;

namespace {

// at least one triangle where a caller has no reason to call with none: Python returns its empty record without a call
int check_triangles(int64_t n_triangles)
{
    if (n_triangles < 0 || n_triangles > tsamd::kQualityMaxTriangles)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "n_triangles out of range (0 .. 715827881: corner ids 3 t + k are 32-bit)");
    return TSAMD_OK;
}

}  // namespace

extern "C" {

int tsamd_quality_info(int32_t *block_out, int32_t *tile_out, int32_t *queue_out)
{
    if (int rc = tsamd::check_not_null({{block_out, "block_out"}, {tile_out, "tile_out"}, {queue_out, "queue_out"}})) return rc;
    *block_out = tsamd::kQualityBlock;
    *tile_out = tsamd::kQualityTile;
    *queue_out = tsamd::kQualityQueue;
    return TSAMD_OK;
}

int tsamd_quality_prepare(const float *v_dev, int64_t n_vertices, const int32_t *faces_dev, int64_t n_triangles, double lo, double hi, uint64_t *corners_out_dev,
                          uint64_t *boxes_out_dev, uint8_t *state_out_dev, double *shape_out_dev, int64_t *morton_out_dev, void *stream)
{
    int rc = check_triangles(n_triangles);
    if (rc) return rc;
    if ((rc = tsamd::check_vertex_count(n_vertices, "faces"))) return rc;
    if ((rc = tsamd::check_cube(lo, hi))) return rc;
    if (n_triangles == 0) return TSAMD_OK;                                 // nothing to write
    if ((rc = check_buffers({{faces_dev, "faces_dev", 4}, {corners_out_dev, "corners_out_dev", 8}, {boxes_out_dev, "boxes_out_dev", 8},
                             {state_out_dev, "state_out_dev", 1}, {shape_out_dev, "shape_out_dev", 8}, {morton_out_dev, "morton_out_dev", 8}})))
        return rc;
    if (n_vertices > 0 && (rc = check_buffers({{v_dev, "v_dev", 4}}))) return rc;
    TSAMD_HIP(tsamd::launch_quality_prepare(v_dev, n_vertices, faces_dev, n_triangles, lo, hi, corners_out_dev, boxes_out_dev, state_out_dev, shape_out_dev,
                                            morton_out_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_quality_pairs(const uint64_t *corners_dev, const uint64_t *boxes_dev, const uint8_t *state_dev, int64_t n_triangles, uint64_t *tile_boxes_dev,
                        int64_t max_pairs, int32_t *crossings_out_dev, int64_t *pairs_out_dev, int64_t *stats_out_dev, void *stream)
{
    int rc = check_triangles(n_triangles);
    if (rc) return rc;
    if (max_pairs < 0 || max_pairs > INT32_MAX) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "max_pairs out of range (0 .. 2^31 - 1)");
    if ((rc = check_buffers({{stats_out_dev, "stats_out_dev", 8}}))) return rc;
    auto stream_ = static_cast<hipStream_t>(stream);
    if (n_triangles == 0) {
        TSAMD_HIP(hipMemsetAsync(stats_out_dev, 0, tsamd::kQualityStats * sizeof(int64_t), stream_));
        return TSAMD_OK;
    }
    if ((rc = check_buffers({{corners_dev, "corners_dev", 8}, {boxes_dev, "boxes_dev", 8}, {state_dev, "state_dev", 1}, {crossings_out_dev, "crossings_out_dev", 4}})))
        return rc;
    if (max_pairs > 0 && (rc = check_buffers({{pairs_out_dev, "pairs_out_dev", 8}}))) return rc;
    if (tile_boxes_dev && (rc = tsamd::check_aligned(tile_boxes_dev, "tile_boxes_dev", 8))) return rc;
    TSAMD_HIP(tsamd::launch_quality_pairs(corners_dev, boxes_dev, state_dev, n_triangles, tile_boxes_dev, max_pairs, crossings_out_dev, pairs_out_dev,
                                          stats_out_dev, stream_));
    return TSAMD_OK;
}

int tsamd_quality_edges(const int32_t *faces_dev, const uint8_t *state_dev, int64_t n_triangles, int64_t n_vertices, int64_t *und_keys_out_dev,
                        int64_t *dir_keys_out_dev, int32_t *vertex_pairs_out_dev, uint8_t *referenced_out_dev, void *stream)
{
    int rc = check_triangles(n_triangles);
    if (rc) return rc;
    if ((rc = tsamd::check_vertex_count(n_vertices, "faces"))) return rc;
    if (n_vertices > 0 && (rc = check_buffers({{referenced_out_dev, "referenced_out_dev", 1}}))) return rc;
    if (n_triangles > 0 && (rc = check_buffers({{faces_dev, "faces_dev", 4}, {state_dev, "state_dev", 1}, {und_keys_out_dev, "und_keys_out_dev", 8},
                                                {dir_keys_out_dev, "dir_keys_out_dev", 8}, {vertex_pairs_out_dev, "vertex_pairs_out_dev", 4}})))
        return rc;
    if (n_triangles == 0) {
        if (n_vertices > 0) TSAMD_HIP(hipMemsetAsync(referenced_out_dev, 0, size_t(n_vertices), static_cast<hipStream_t>(stream)));
        return TSAMD_OK;
    }
    TSAMD_HIP(tsamd::launch_quality_edges(faces_dev, state_dev, n_triangles, n_vertices, und_keys_out_dev, dir_keys_out_dev, vertex_pairs_out_dev,
                                          referenced_out_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_quality_fan_pairs(const int32_t *faces_dev, int64_t n_triangles, const int64_t *sorted_keys_dev, const int64_t *order_dev,
                            int32_t *corner_pairs_out_dev, void *stream)
{
    int rc = check_triangles(n_triangles);
    if (rc) return rc;
    if (n_triangles == 0) return TSAMD_OK;
    if ((rc = check_buffers({{faces_dev, "faces_dev", 4}, {sorted_keys_dev, "sorted_keys_dev", 8}, {order_dev, "order_dev", 8},
                             {corner_pairs_out_dev, "corner_pairs_out_dev", 4}})))
        return rc;
    TSAMD_HIP(tsamd::launch_quality_fan_pairs(faces_dev, n_triangles, sorted_keys_dev, order_dev, corner_pairs_out_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_quality_union(const int32_t *pairs_dev, int64_t n_pairs, int32_t *labels_out_dev, int64_t n, void *workspace_dev, int64_t *rounds_out, void *stream)
{
    if (n < 0 || n > INT32_MAX) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "n out of range (0 .. 2^31 - 1)");
    if (n_pairs < 0 || n_pairs > INT32_MAX) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "n_pairs out of range (0 .. 2^31 - 1)");
    if (rounds_out) *rounds_out = 0;
    if (n == 0) return TSAMD_OK;
    int rc = check_buffers({{labels_out_dev, "labels_out_dev", 4}, {workspace_dev, "workspace_dev", 4}});
    if (rc) return rc;
    if (n_pairs > 0 && (rc = check_buffers({{pairs_dev, "pairs_dev", 4}}))) return rc;
    // every round but the last joins two roots at least: n - 1 rounds that change something, and one that finds nothing to do
    const int64_t cap = n + 1;
    int32_t converged = 0;
    int64_t rounds = 0;
    TSAMD_HIP(tsamd::launch_quality_union(pairs_dev, n_pairs, labels_out_dev, n, static_cast<int32_t *>(workspace_dev), cap, &converged, &rounds,
                                          static_cast<hipStream_t>(stream)));
    if (rounds_out) *rounds_out = rounds;
    if (!converged) return capi_fail(TSAMD_ERR_HIP, "the union-find did not settle within n + 1 rounds: a logic error in csrc/quality_kernels.hip");
    return TSAMD_OK;
}

}  // extern "C"
