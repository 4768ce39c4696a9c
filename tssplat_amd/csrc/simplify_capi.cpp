// C ABI of the surface simplifier (include/tssplat_amd.h, tsamd_simplify_keys / _cells / _faces / _dedupe): stateless entry points over
// caller-owned buffers.  Every argument is checked before the first device call.
#include "capi_common.h"
#include "simplify.h"

using tsamd::capi_fail;
using tsamd::check_buffers;

namespace {

int check_triangle_count(int64_t n_triangles)
{
    if (n_triangles < 0 || n_triangles > tsamd::kSimplifyMaxTriangles)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "n_triangles out of range (0 .. (2^31 - 1) / 3: three record slots per triangle)");
    return TSAMD_OK;
}

// what tsamd_simplify_keys and tsamd_simplify_cells share: the sizes, then the cell grid
int check_sizes(int64_t n_vertices, int64_t n_triangles, int32_t cells, double lo, double hi)
{
    int rc = tsamd::check_vertex_count(n_vertices, "faces");
    if (rc || (rc = check_triangle_count(n_triangles)) || (rc = tsamd::check_grid(cells, 1, tsamd::kSimplifyMaxCells, "cells"))) return rc;
    return tsamd::check_cube(lo, hi, cells, "cells");
}

}  // namespace

extern "C" {

int tsamd_simplify_keys(const float *v_dev, int64_t n_vertices, const int32_t *faces_dev, int64_t n_triangles, int32_t cells, double lo, double hi,
                        int32_t *vkey_out_dev, int64_t *records_out_dev, uint8_t *state_out_dev, void *stream)
{
    int rc = check_sizes(n_vertices, n_triangles, cells, lo, hi);
    if (rc) return rc;
    if (n_vertices > 0 && (rc = check_buffers({{v_dev, "v_dev", 4}, {vkey_out_dev, "vkey_out_dev", 4}}))) return rc;
    if (n_triangles > 0 && (rc = check_buffers({{faces_dev, "faces_dev", 4}, {records_out_dev, "records_out_dev", 8}, {state_out_dev, "state_out_dev", 1}}))) return rc;
    TSAMD_HIP(tsamd::launch_simplify_keys(v_dev, n_vertices, faces_dev, n_triangles, cells, lo, hi, vkey_out_dev, records_out_dev, state_out_dev,
                                          static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_simplify_cells(const float *v_dev, int64_t n_vertices, const int32_t *faces_dev, int64_t n_triangles, int32_t cells, double lo, double hi,
                         int32_t placement, double stabilise, const int32_t *vkey_dev, const int64_t *records_dev, const int64_t *perm_dev, float *pos_out_dev,
                         uint8_t *head_out_dev, int32_t *run_out_dev, int32_t *status_out_dev, void *stream)
{
    int rc = check_sizes(n_vertices, n_triangles, cells, lo, hi);
    if (rc) return rc;
    if (placement != tsamd::kSimplifyQuadric && placement != tsamd::kSimplifyMean)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "placement must be TSAMD_SIMPLIFY_QUADRIC (0) or TSAMD_SIMPLIFY_MEAN (1)");
    if (!(std::isfinite(stabilise) && stabilise >= 0.0)) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "stabilise must be a finite number >= 0");
    if ((rc = check_buffers({{status_out_dev, "status_out_dev", 4}}))) return rc;
    if (n_vertices > 0 && (rc = check_buffers({{v_dev, "v_dev", 4}, {vkey_dev, "vkey_dev", 4}}))) return rc;
    if (n_triangles > 0 && (rc = check_buffers({{faces_dev, "faces_dev", 4}, {records_dev, "records_dev", 8}, {perm_dev, "perm_dev", 8}, {pos_out_dev, "pos_out_dev", 4},
                                                {head_out_dev, "head_out_dev", 1}, {run_out_dev, "run_out_dev", 4}})))
        return rc;
    TSAMD_HIP(tsamd::launch_simplify_cells(v_dev, n_vertices, faces_dev, n_triangles, cells, lo, hi, placement, stabilise, vkey_dev, records_dev, perm_dev,
                                           pos_out_dev, head_out_dev, run_out_dev, status_out_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_simplify_faces(const int32_t *run_dev, const uint8_t *state_dev, int64_t n_triangles, int32_t *tri_out_dev, int64_t *key_ab_out_dev,
                         int64_t *key_c_out_dev, void *stream)
{
    int rc = check_triangle_count(n_triangles);
    if (rc) return rc;
    if (n_triangles == 0) return TSAMD_OK;                                 // nothing to write
    if ((rc = check_buffers({{run_dev, "run_dev", 4}, {state_dev, "state_dev", 1}, {tri_out_dev, "tri_out_dev", 4}, {key_ab_out_dev, "key_ab_out_dev", 8},
                             {key_c_out_dev, "key_c_out_dev", 8}})))
        return rc;
    TSAMD_HIP(tsamd::launch_simplify_faces(run_dev, state_dev, n_triangles, tri_out_dev, key_ab_out_dev, key_c_out_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_simplify_dedupe(const int32_t *tri_dev, const int64_t *order_dev, int64_t n_triangles, uint8_t *keep_out_dev, uint8_t *used_out_dev,
                          int32_t *status_out_dev, void *stream)
{
    int rc = check_triangle_count(n_triangles);
    if (rc || (rc = check_buffers({{status_out_dev, "status_out_dev", 4}}))) return rc;
    if (n_triangles > 0 && (rc = check_buffers({{tri_dev, "tri_dev", 4}, {order_dev, "order_dev", 8}, {keep_out_dev, "keep_out_dev", 1}, {used_out_dev, "used_out_dev", 1}})))
        return rc;
    TSAMD_HIP(tsamd::launch_simplify_dedupe(tri_dev, order_dev, n_triangles, keep_out_dev, used_out_dev, status_out_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

}  // extern "C"
