"""Float64 numpy restatement of ``dr.texture`` (include/tssplat_amd.h, "texture sampling"), forward and backward.

tex [TB (1 or B), H, W, C], uv [B, h, w, 2] -> out [B, h, w, C].  x = u W - 0.5, y = v H - 0.5, no flip.  'linear' takes the
taps at floor(x), floor(x) + 1 and likewise in y with the fractional parts as weights; 'nearest' takes texel floor(u W),
floor(v H).  'wrap' reduces tap indices by a true modulo, 'clamp' clamps them, 'zero' gives out-of-range taps the value 0.
Backward: grad_tex gets weight x g at every tap that exists, summed over the batch when TB = 1; grad_uv (linear only) is
dL/du = W sum_c g_c ((t10 - t00)(1 - fy) + (t11 - t01) fy), dL/dv = H sum_c g_c ((t01 - t00)(1 - fx) + (t11 - t10) fx), from
the taps actually used.  uv is taken as given (float32 values are converted exactly); everything else runs in float64.
"""
import numpy as np


def _resolve(idx, n, boundary):
    """(index in [0, n), exists) of tap idx along an axis of n texels."""
    if boundary == "wrap":
        return np.mod(idx, n), np.ones(idx.shape, bool)
    clamped = np.clip(idx, 0, n - 1)
    if boundary == "clamp":
        return clamped, np.ones(idx.shape, bool)
    assert boundary == "zero"
    return clamped, clamped == idx


def _taps(tex_shape, uv, filter_mode, boundary):
    """A list of (batch index into tex, row, column, exists, weight, d weight/dx-part) taps per pixel; plus (fx, fy)."""
    TB, H, W, _ = tex_shape
    uv = np.asarray(uv, np.float64)
    B = uv.shape[0]
    tb = np.broadcast_to((np.arange(B) if TB > 1 else np.zeros(B, np.int64))[:, None, None], uv.shape[:3])
    u, v = uv[..., 0], uv[..., 1]
    if filter_mode == "nearest":
        rx, ex = _resolve(np.floor(u * W).astype(np.int64), W, boundary)
        ry, ey = _resolve(np.floor(v * H).astype(np.int64), H, boundary)
        return tb, [(ry, rx, ex & ey, np.ones(u.shape))], None
    assert filter_mode == "linear"
    x, y = u * W - 0.5, v * H - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    taps = []
    for dy, wy in ((0, 1 - fy), (1, fy)):
        for dx, wx in ((0, 1 - fx), (1, fx)):
            rx, ex = _resolve(x0 + dx, W, boundary)
            ry, ey = _resolve(y0 + dy, H, boundary)
            taps.append((ry, rx, ex & ey, wx * wy))
    return tb, taps, (fx, fy)                                    # tap order: 00, 10, 01, 11 (x first)


def forward(tex, uv, filter_mode="linear", boundary="wrap"):
    tex = np.asarray(tex, np.float64)
    tb, taps, _ = _taps(tex.shape, uv, filter_mode, boundary)
    out = 0.0
    for ry, rx, exists, w in taps:
        out = out + (w * exists)[..., None] * tex[tb, ry, rx]
    return out


def backward(tex, uv, grad_out, filter_mode="linear", boundary="wrap"):
    """(grad_tex [tex's shape], grad_uv [uv's shape] or None for 'nearest', abs_adds [tex's shape], n_adds [tex's shape]):
    abs_adds is sum |w g| and n_adds the number of non-zero contributions per texture element (what a rounding bound needs)."""
    tex, g = np.asarray(tex, np.float64), np.asarray(grad_out, np.float64)
    TB, H, W, Cn = tex.shape
    tb, taps, frac = _taps(tex.shape, uv, filter_mode, boundary)
    grad_tex, abs_adds, n_adds = np.zeros_like(tex), np.zeros_like(tex), np.zeros_like(tex)
    for ry, rx, exists, w in taps:
        wg = (w * exists)[..., None] * g
        np.add.at(grad_tex, (tb, ry, rx), wg)
        np.add.at(abs_adds, (tb, ry, rx), np.abs(wg))
        np.add.at(n_adds, (tb, ry, rx), ((w * exists) != 0)[..., None] * np.ones(Cn))
    if filter_mode == "nearest":
        return grad_tex, None, abs_adds, n_adds
    fx, fy = frac
    t00, t10, t01, t11 = (exists[..., None] * tex[tb, ry, rx] for ry, rx, exists, _ in taps)
    du = W * np.sum(g * ((t10 - t00) * (1 - fy)[..., None] + (t11 - t01) * fy[..., None]), axis=-1)
    dv = H * np.sum(g * ((t01 - t00) * (1 - fx)[..., None] + (t11 - t10) * fx[..., None]), axis=-1)
    return grad_tex, np.stack([du, dv], -1), abs_adds, n_adds
