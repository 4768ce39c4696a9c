// C ABI of the sphere initialisation (include/tssplat_amd.h, tsamd_hull_carve / tsamd_edt_squared / tsamd_greedy_cover): stateless
// entry points over caller-owned buffers.  Every argument is checked before the first device call.
#include "capi_common.h"
#include "init.h"

using tsamd::capi_fail;
using tsamd::check_not_null;

extern "C" {

int tsamd_hull_carve(const float *alpha_dev, int64_t batch, int32_t height, int32_t width, int32_t channels, int32_t channel, float threshold,
                     const float *mvp_dev, int32_t grid, double lo, double hi, uint32_t *bits_workspace_dev, uint8_t *hull_out_dev, void *stream)
{
    int rc = tsamd::check_grid(grid, 1, tsamd::kInitMaxGrid);
    if (rc || (rc = tsamd::check_image(batch, height, width, false))) return rc;
    if (channels < 0) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "channels is negative");
    if (channel < 0 || channel >= channels) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "channel out of range (0 .. channels - 1)");
    if (batch > 0 && (height == 0 || width == 0)) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "height and width must be at least 1 when batch is not 0");
    // one workgroup packs four 64-pixel pieces of image rows
    if (batch > INT32_MAX || batch * height * int64_t((width + 63) / 64) > 4 * int64_t(INT32_MAX))
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "batch x height x ceil(width / 64) exceeds the grid limit (2^31 - 1 workgroups of four)");
    if ((rc = tsamd::check_cube(lo, hi))) return rc;
    if (batch > 0 && (rc = check_not_null({{alpha_dev, "alpha_dev"}, {mvp_dev, "mvp_dev"}, {bits_workspace_dev, "bits_workspace_dev"}}))) return rc;
    if ((rc = check_not_null({{hull_out_dev, "hull_out_dev"}}))) return rc;
    TSAMD_HIP(tsamd::launch_hull_carve(alpha_dev, batch, height, width, channels, channel, threshold, mvp_dev, grid, lo, (hi - lo) / grid, bits_workspace_dev,
                                       hull_out_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_edt_squared(const uint8_t *mask_dev, int32_t grid, int32_t *workspace_dev, int32_t *d2_out_dev, int32_t *status_out_dev, void *stream)
{
    int rc = tsamd::check_grid(grid, 1, tsamd::kInitMaxGrid);
    if (rc || (rc = check_not_null({{mask_dev, "mask_dev"}, {workspace_dev, "workspace_dev"}, {d2_out_dev, "d2_out_dev"}, {status_out_dev, "status_out_dev"}})))
        return rc;
    TSAMD_HIP(tsamd::launch_edt_squared(mask_dev, grid, workspace_dev, d2_out_dev, status_out_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_greedy_cover(const uint8_t *hull_dev, const int32_t *d2_dev, int32_t grid, int32_t n_spheres, double s2, double hs2, double m2,
                       void *workspace_dev, uint8_t *uncovered_out_dev, int32_t *flat_out_dev, int32_t *q_out_dev, int32_t *count_out_dev, void *stream)
{
    int rc = tsamd::check_grid(grid, 1, tsamd::kInitMaxGrid);
    if (rc) return rc;
    if (n_spheres < 0 || n_spheres > (1 << 20)) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "n_spheres out of range (0 .. 2^20)");
    if (!(s2 >= 0.0) || !(hs2 >= 0.0) || !(m2 >= 0.0)) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "s2, hs2 and m2 are squares: none may be negative or NaN");
    if ((rc = check_not_null({{hull_dev, "hull_dev"}, {d2_dev, "d2_dev"}, {workspace_dev, "workspace_dev"}, {uncovered_out_dev, "uncovered_out_dev"},
                              {count_out_dev, "count_out_dev"}})))
        return rc;
    if (n_spheres > 0 && (rc = check_not_null({{flat_out_dev, "flat_out_dev"}, {q_out_dev, "q_out_dev"}}))) return rc;
    TSAMD_HIP(tsamd::launch_greedy_cover(hull_dev, d2_dev, grid, n_spheres, s2, hs2, m2, static_cast<unsigned long long *>(workspace_dev), uncovered_out_dev,
                                         flat_out_dev, q_out_dev, count_out_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

}  // extern "C"
