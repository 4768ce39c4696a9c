// C ABI of the surface smoother (include/tssplat_amd.h, tsamd_smooth_*): stateless entry points over caller-owned buffers.
// Every argument is checked before the first device call; nothing synchronises the host.
#include "capi_common.h"
#include "smooth.h"

using tsamd::capi_fail;
using tsamd::check_buffers;

namespace {

int check_triangles(int64_t n_triangles)
{
    if (n_triangles < 0 || n_triangles > tsamd::kSmoothMaxTriangles)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "n_triangles out of range (0 .. 357913940: six directed keys per face, positions are 32-bit)");
    return TSAMD_OK;
}

// The sizes and pointers of a tsamd_smooth_mesh, composed of the shared checks; the lists of faces only where the mode walks them.
int check_mesh(const tsamd_smooth_mesh *mesh, bool with_faces, tsamd::SmoothMesh *out)
{
    if (int rc = tsamd::check_not_null({{mesh, "mesh"}})) return rc;
    if (mesh->struct_size != int32_t(sizeof(tsamd_smooth_mesh))) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "mesh->struct_size is not sizeof(tsamd_smooth_mesh)");
    int rc = tsamd::check_vertex_count(mesh->n_vertices, "faces");
    if (rc) return rc;
    if ((rc = check_triangles(mesh->n_triangles))) return rc;
    if (mesh->n_neighbours < 0 || mesh->n_neighbours > INT32_MAX) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "mesh->n_neighbours out of range (0 .. 2^31 - 1)");
    if (mesh->n_face_entries < 0 || mesh->n_face_entries > INT32_MAX)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "mesh->n_face_entries out of range (0 .. 2^31 - 1)");
    *out = tsamd::SmoothMesh{mesh->offsets_dev,  mesh->neighbours_dev,  mesh->n_neighbours, mesh->face_offsets_dev, mesh->faces_of_dev,
                             mesh->n_face_entries, mesh->faces_dev, mesh->n_triangles, mesh->n_vertices};
    if (mesh->n_vertices == 0) return TSAMD_OK;
    if ((rc = check_buffers({{mesh->offsets_dev, "mesh->offsets_dev", 4}}))) return rc;
    if (mesh->n_neighbours > 0 && (rc = check_buffers({{mesh->neighbours_dev, "mesh->neighbours_dev", 4}}))) return rc;
    if (!with_faces) return TSAMD_OK;
    if ((rc = check_buffers({{mesh->face_offsets_dev, "mesh->face_offsets_dev", 4}}))) return rc;
    if (mesh->n_face_entries > 0 && (rc = check_buffers({{mesh->faces_of_dev, "mesh->faces_of_dev", 4}}))) return rc;
    if (mesh->n_triangles > 0 && (rc = check_buffers({{mesh->faces_dev, "mesh->faces_dev", 4}}))) return rc;
    return TSAMD_OK;
}

int check_step(int32_t stride, int32_t mode, double max_move, const float *v0_dev)
{
    if (stride != 3 && stride != 4) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "stride must be 3 or 4 (float64 per record)");
    if (mode != TSAMD_SMOOTH_TAUBIN && mode != TSAMD_SMOOTH_TANGENTIAL) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "mode must be TSAMD_SMOOTH_TAUBIN or TSAMD_SMOOTH_TANGENTIAL");
    if (v0_dev && !(std::isfinite(max_move) && max_move >= 0.0)) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "max_move must be finite and >= 0");
    if (v0_dev) return tsamd::check_aligned(v0_dev, "v0_dev", 4);
    return TSAMD_OK;
}

}  // namespace

extern "C" {

int tsamd_smooth_keys(const int32_t *faces_dev, int64_t n_triangles, int64_t n_vertices, uint8_t *valid_out_dev, int64_t *edge_keys_out_dev,
                      int64_t *face_keys_out_dev, void *stream)
{
    int rc = check_triangles(n_triangles);
    if (rc) return rc;
    if ((rc = tsamd::check_vertex_count(n_vertices, "faces"))) return rc;
    if (n_triangles == 0) return TSAMD_OK;                                 // nothing to write
    if ((rc = check_buffers({{faces_dev, "faces_dev", 4}, {valid_out_dev, "valid_out_dev", 1}, {edge_keys_out_dev, "edge_keys_out_dev", 8},
                             {face_keys_out_dev, "face_keys_out_dev", 8}})))
        return rc;
    TSAMD_HIP(tsamd::launch_smooth_keys(faces_dev, n_triangles, n_vertices, valid_out_dev, edge_keys_out_dev, face_keys_out_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_smooth_rows(const int64_t *sorted_keys_dev, int64_t n_keys, int64_t n_vertices, uint8_t *head_out_dev, uint8_t *irregular_out_dev, void *stream)
{
    if (n_keys < 0 || n_keys > INT32_MAX) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "n_keys out of range (0 .. 2^31 - 1)");
    int rc = tsamd::check_vertex_count(n_vertices, "faces");
    if (rc) return rc;
    if (n_vertices > 0 && (rc = check_buffers({{irregular_out_dev, "irregular_out_dev", 1}}))) return rc;
    if (n_keys > 0 && (rc = check_buffers({{sorted_keys_dev, "sorted_keys_dev", 8}, {head_out_dev, "head_out_dev", 1}}))) return rc;
    TSAMD_HIP(tsamd::launch_smooth_rows(sorted_keys_dev, n_keys, n_vertices, head_out_dev, irregular_out_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_smooth_classify(const float *v_dev, const tsamd_smooth_mesh *mesh, const uint8_t *irregular_dev, const uint8_t *pinned_dev, int32_t boundary,
                          uint8_t *class_out_dev, void *stream)
{
    tsamd::SmoothMesh m{};
    int rc = check_mesh(mesh, false, &m);
    if (rc) return rc;
    if (boundary != TSAMD_SMOOTH_BOUNDARY_FIXED && boundary != TSAMD_SMOOTH_BOUNDARY_FREE)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "boundary must be TSAMD_SMOOTH_BOUNDARY_FIXED or TSAMD_SMOOTH_BOUNDARY_FREE");
    if (m.n_vertices == 0) return TSAMD_OK;
    if ((rc = check_buffers({{v_dev, "v_dev", 4}, {irregular_dev, "irregular_dev", 1}, {class_out_dev, "class_out_dev", 1}}))) return rc;
    TSAMD_HIP(tsamd::launch_smooth_classify(v_dev, m, irregular_dev, pinned_dev, boundary == TSAMD_SMOOTH_BOUNDARY_FREE, class_out_dev,
                                            static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_smooth_step(const double *src_dev, double *dst_dev, int32_t stride, const tsamd_smooth_mesh *mesh, const uint8_t *class_dev, int32_t mode, double coef,
                      const float *v0_dev, double max_move, void *stream)
{
    int rc = check_step(stride, mode, max_move, v0_dev);
    if (rc) return rc;
    tsamd::SmoothMesh m{};
    if ((rc = check_mesh(mesh, mode == TSAMD_SMOOTH_TANGENTIAL, &m))) return rc;
    if (m.n_vertices == 0) return TSAMD_OK;
    const uintptr_t align = stride == 4 ? 32 : 8;
    if ((rc = check_buffers({{src_dev, "src_dev", align}, {dst_dev, "dst_dev", align}, {class_dev, "class_dev", 1}}))) return rc;
    if (src_dev == dst_dev) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "dst_dev must be another buffer than src_dev (a half-step reads only the state before it)");
    TSAMD_HIP(tsamd::launch_smooth_step(src_dev, dst_dev, stride, m, class_dev, mode, coef, v0_dev, max_move, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_smooth_run(double *state_a_dev, double *state_b_dev, int32_t stride, const tsamd_smooth_mesh *mesh, const uint8_t *class_dev, int32_t mode, double lam,
                     double mu, int32_t iterations, const float *v0_dev, double max_move, int32_t *result_in_b_out, void *stream)
{
    int rc = check_step(stride, mode, max_move, v0_dev);
    if (rc) return rc;
    if (iterations < 0 || iterations > tsamd::kSmoothMaxIterations) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "iterations out of range (0 .. 4096)");
    if (std::isnan(lam) || std::isnan(mu)) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "lam / mu is NaN");
    if ((rc = tsamd::check_not_null({{result_in_b_out, "result_in_b_out"}}))) return rc;
    tsamd::SmoothMesh m{};
    if ((rc = check_mesh(mesh, mode == TSAMD_SMOOTH_TANGENTIAL, &m))) return rc;
    *result_in_b_out = 0;
    if (m.n_vertices == 0) return TSAMD_OK;
    const uintptr_t align = stride == 4 ? 32 : 8;
    if ((rc = check_buffers({{state_a_dev, "state_a_dev", align}, {state_b_dev, "state_b_dev", align}, {class_dev, "class_dev", 1}}))) return rc;
    if (state_a_dev == state_b_dev) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "state_b_dev must be another buffer than state_a_dev");
    // a half-step whose coefficient is exactly zero is skipped; tangential relaxation has one half-step per iteration
    const double coef[2] = {lam, mu};
    const int n_coef = mode == TSAMD_SMOOTH_TAUBIN ? 2 : 1;
    double *src = state_a_dev, *dst = state_b_dev;
    for (int32_t it = 0; it < iterations; ++it)
        for (int k = 0; k < n_coef; ++k) {
            if (coef[k] == 0.0) continue;
            TSAMD_HIP(tsamd::launch_smooth_step(src, dst, stride, m, class_dev, mode, coef[k], v0_dev, max_move, static_cast<hipStream_t>(stream)));
            double *t = src;
            src = dst;
            dst = t;
        }
    *result_in_b_out = src == state_b_dev ? 1 : 0;
    return TSAMD_OK;
}

}  // extern "C"
