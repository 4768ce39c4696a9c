// C ABI of the fully fused MLP (include/tssplat_amd.h, "fully fused MLP" section): the host-side layout, the workspace size and
// the stateless forward / backward entry points.  The caller owns every buffer and names the device by making it current.
#include <cstdint>
#include <string>

#include "capi_common.h"
#include "mlp.h"

using tsamd::capi_fail;

namespace tsamd {

bool mlp_layout(int32_t n_in, int32_t n_out, int32_t width, int32_t n_hidden, int32_t act, int32_t out_act, MlpShape &s,
                std::string &err)
{
    if (width != 16 && width != 32 && width != 64 && width != 128) {
        err = "n_neurons must be 16, 32, 64 or 128";
        return false;
    }
    if (n_hidden < 1 || n_hidden > kMlpMaxHidden) {
        err = "n_hidden_layers must be 1 .. " + std::to_string(kMlpMaxHidden);
        return false;
    }
    if (n_in < 1 || n_in > 256) {
        err = "n_input_dims must be 1 .. 256";
        return false;
    }
    if (n_out < 1 || n_out > 64) {
        err = "n_output_dims must be 1 .. 64";
        return false;
    }
    if (act != TSAMD_MLP_ACT_NONE && act != TSAMD_MLP_ACT_RELU) {
        err = "activation must be TSAMD_MLP_ACT_NONE or TSAMD_MLP_ACT_RELU";
        return false;
    }
    if (out_act != TSAMD_MLP_ACT_NONE && out_act != TSAMD_MLP_ACT_SIGMOID) {
        err = "output_activation must be TSAMD_MLP_ACT_NONE or TSAMD_MLP_ACT_SIGMOID";
        return false;
    }
    s = MlpShape{};
    s.width = width;
    s.n_hidden = n_hidden;
    s.n_in = n_in;
    s.n_out = n_out;
    s.in_w = (n_in + 15) / 16 * 16;
    s.out_w = (n_out + 15) / 16 * 16;
    s.act = act;
    s.out_act = out_act;
    int64_t off = 0;
    for (int m = 0; m <= n_hidden; ++m) {
        s.rows[m] = m == n_hidden ? s.out_w : width;
        s.cols[m] = m == 0 ? s.in_w : width;
        s.off[m] = off;
        off += int64_t(s.rows[m]) * s.cols[m];
    }
    s.off[n_hidden + 1] = off;
    s.n_params = off;
    return true;
}

}  // namespace tsamd

namespace {

int layout_or_fail(int32_t n_in, int32_t n_out, int32_t width, int32_t n_hidden, int32_t act, int32_t out_act, tsamd::MlpShape &s)
{
    std::string err;
    if (!tsamd::mlp_layout(n_in, n_out, width, n_hidden, act, out_act, s, err))
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "fused MLP: " + err);
    return TSAMD_OK;
}

int check_rows(int64_t n_rows, const void *x_dev, const void *params_dev)
{
    if (n_rows < 0) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "fused MLP: n_rows < 0");
    if (n_rows > (int64_t(1) << 40)) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "fused MLP: n_rows above 2^40");
    if (n_rows > 0 && !x_dev) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "fused MLP: x_dev is null");
    if (n_rows > 0 && !params_dev) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "fused MLP: params_dev is null");
    if (reinterpret_cast<uintptr_t>(x_dev) % 4 || reinterpret_cast<uintptr_t>(params_dev) % 4)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "fused MLP: x_dev / params_dev not float-aligned");
    return TSAMD_OK;
}

}  // namespace

extern "C" {

int tsamd_mlp_layout(int32_t n_input_dims, int32_t n_output_dims, int32_t n_neurons, int32_t n_hidden_layers, int32_t activation,
                     int32_t output_activation, int64_t *n_params_out, int32_t *in_width_out, int32_t *out_width_out)
{
    tsamd::MlpShape s;
    const int rc = layout_or_fail(n_input_dims, n_output_dims, n_neurons, n_hidden_layers, activation, output_activation, s);
    if (rc) return rc;
    if (n_params_out) *n_params_out = s.n_params;
    if (in_width_out) *in_width_out = s.in_w;
    if (out_width_out) *out_width_out = s.out_w;
    return TSAMD_OK;
}

int64_t tsamd_mlp_workspace_bytes(int64_t n_rows, int32_t n_input_dims, int32_t n_output_dims, int32_t n_neurons,
                                  int32_t n_hidden_layers, int32_t activation, int32_t output_activation)
{
    tsamd::MlpShape s;
    if (layout_or_fail(n_input_dims, n_output_dims, n_neurons, n_hidden_layers, activation, output_activation, s)) return -1;
    if (n_rows < 0 || n_rows > (int64_t(1) << 40)) {
        capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "fused MLP: n_rows must be 0 .. 2^40");
        return -1;
    }
    return tsamd::mlp_workspace_bytes(s, n_rows);
}

int tsamd_mlp_forward(const float *x_dev, int64_t n_rows, const float *params_dev, int32_t n_input_dims, int32_t n_output_dims,
                      int32_t n_neurons, int32_t n_hidden_layers, int32_t activation, int32_t output_activation, float *y_dev, void *stream)
{
    tsamd::MlpShape s;
    int rc = layout_or_fail(n_input_dims, n_output_dims, n_neurons, n_hidden_layers, activation, output_activation, s);
    if (rc) return rc;
    rc = check_rows(n_rows, x_dev, params_dev);
    if (rc) return rc;
    if (n_rows > 0 && !y_dev) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "fused MLP: y_dev is null");
    if (reinterpret_cast<uintptr_t>(y_dev) % 4) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "fused MLP: y_dev is not float-aligned");
    if (n_rows == 0) return TSAMD_OK;
    TSAMD_HIP(tsamd::launch_mlp_forward(x_dev, n_rows, params_dev, s, y_dev, static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

int tsamd_mlp_backward(const float *x_dev, int64_t n_rows, const float *params_dev, int32_t n_input_dims, int32_t n_output_dims,
                       int32_t n_neurons, int32_t n_hidden_layers, int32_t activation, int32_t output_activation,
                       const float *grad_y_dev, float *grad_params_dev, float *grad_x_dev, void *workspace_dev, void *stream)
{
    tsamd::MlpShape s;
    int rc = layout_or_fail(n_input_dims, n_output_dims, n_neurons, n_hidden_layers, activation, output_activation, s);
    if (rc) return rc;
    rc = check_rows(n_rows, x_dev, params_dev);
    if (rc) return rc;
    if (n_rows > 0 && !grad_y_dev) return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "fused MLP: grad_y_dev is null");
    if (n_rows > 0 && grad_params_dev && !workspace_dev)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "fused MLP: workspace_dev is null (tsamd_mlp_workspace_bytes)");
    if (reinterpret_cast<uintptr_t>(grad_y_dev) % 4 || reinterpret_cast<uintptr_t>(grad_params_dev) % 4 ||
        reinterpret_cast<uintptr_t>(grad_x_dev) % 4 || reinterpret_cast<uintptr_t>(workspace_dev) % 4)
        return capi_fail(TSAMD_ERR_INVALID_ARGUMENT, "fused MLP: a buffer is not float-aligned");
    if (n_rows == 0) return TSAMD_OK;
    TSAMD_HIP(tsamd::launch_mlp_backward(x_dev, n_rows, params_dev, s, grad_y_dev, grad_params_dev, grad_x_dev,
                                         static_cast<float *>(workspace_dev), static_cast<hipStream_t>(stream)));
    return TSAMD_OK;
}

}  // extern "C"
