"""Float64 numpy oracle of the fully fused MLP (tssplat_amd/network.py, csrc/mlp_kernels.hip).

The network is tiny-cuda-nn's ``FullyFusedMLP`` (its published ``networks/fully_fused_mlp.cu`` and torch binding), restated
rule by rule:

* config: ``n_neurons`` W in {16, 32, 64, 128}, ``n_hidden_layers`` L in 1 .. 8, ``activation`` ReLU / None, ``output_activation``
  None / Sigmoid, 1 .. 256 inputs, 1 .. 64 outputs;
* bias-free; ``in_w = next_multiple(n_input_dims, 16)``, ``out_w = next_multiple(n_output_dims, 16)``; ``params`` is one flat
  float32 vector of L + 1 row-major [out, in] matrices: [W, in_w], (L - 1) x [W, W], [out_w, W];
* padded input columns read 1.0 (the first matrix's padded columns act as a bias); padded output rows are computed and
  discarded;
* forward per row: ``a0 = fp16(x)`` (1.0 in the padded columns), ``a_l = fp16(act(sum_k fp16(W_l[j, k]) a_{l-1}[k]))``,
  ``y = out_act(sum_k fp16(W_out[j, k]) a_L[k])`` returned as float32 (tiny-cuda-nn returns half);
* backward with the loss scale S = 128 of tiny-cuda-nn's torch binding: ``delta_out = fp16(S dy out_act'(z))`` (Sigmoid' from
  y), ``delta_l = fp16((sum_j fp16(W_{l+1}[j, k]) delta_{l+1}[j]) act'(a_l))`` with ReLU' = ``a_l > 0`` on the stored fp16
  value, ``dW_l = (sum over rows of delta_l (x) a_{l-1}) / S``, ``dx = (sum_j fp16(W_1[j, k]) delta_1[j]) / S`` on the real input
  columns; padded output rows get a zero gradient.

PARITY UNPINNED: tiny-cuda-nn is a CUDA-only library; this file is the definition the HIP kernels are tested against.  The
kernels sum in fp32 (MFMA) where the oracle sums in float64; ``exact=True`` drops every fp16 rounding (for the finite-difference
and ``nn.Linear`` self-checks).
"""
from __future__ import annotations

import numpy as np

LOSS_SCALE = 128.0


def _next_multiple(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def layout(n_in: int, n_out: int, width: int, n_hidden: int) -> dict:
    in_w, out_w = _next_multiple(n_in, 16), _next_multiple(n_out, 16)
    shapes = [(width, in_w)] + [(width, width)] * (n_hidden - 1) + [(out_w, width)]
    return {"in_w": in_w, "out_w": out_w, "shapes": shapes, "n_params": sum(r * c for r, c in shapes)}


def split(params: np.ndarray, lay: dict) -> list:
    mats, off = [], 0
    for r, c in lay["shapes"]:
        mats.append(np.asarray(params[off:off + r * c], np.float64).reshape(r, c))
        off += r * c
    return mats


def _h(v, exact):
    return v if exact else np.asarray(v, np.float64).astype(np.float16).astype(np.float64)


def _act(v, act):
    return np.maximum(v, 0.0) if act == "relu" else v


def forward(x, params, n_out, width, n_hidden, act="relu", out_act="none", exact=False) -> dict:
    """``y`` [N, n_out] and the intermediates: ``a`` (a_0 .. a_L), ``z`` (output pre-activation, [N, out_w]), ``mats``
    (the fp16-rounded matrices), ``yfull`` (y over out_w)."""
    x = np.asarray(x, np.float64) if exact else np.asarray(x, np.float32).astype(np.float64)   # the binding casts x to float32
    N, n_in = x.shape
    lay = layout(n_in, n_out, width, n_hidden)
    mats = [_h(m, exact) for m in split(params, lay)]
    a0 = np.ones((N, lay["in_w"]))
    a0[:, :n_in] = x
    a = [_h(a0, exact)]
    for m in mats[:-1]:
        a.append(_h(_act(a[-1] @ m.T, act), exact))
    z = a[-1] @ mats[-1].T
    yfull = 1.0 / (1.0 + np.exp(-z)) if out_act == "sigmoid" else z
    return {"y": yfull[:, :n_out], "yfull": yfull, "z": z, "a": a, "mats": mats, "lay": lay}


def backward(x, params, dy, n_out, width, n_hidden, act="relu", out_act="none", exact=False) -> dict:
    """``dparams`` (flat, float64) and ``dx`` [N, n_in], plus ``deltas`` (delta_0 .. delta_L, scaled by S) and ``f``."""
    f = forward(x, params, n_out, width, n_hidden, act, out_act, exact)
    N = f["z"].shape[0]
    n_in = np.asarray(x).shape[1]
    g = np.zeros((N, f["lay"]["out_w"]))
    g[:, :n_out] = LOSS_SCALE * np.asarray(dy, np.float64)
    if out_act == "sigmoid":
        g = g * (f["yfull"] * (1.0 - f["yfull"]))
    delta = _h(g, exact)
    mats, a = f["mats"], f["a"]
    grads = [None] * len(mats)
    deltas = [None] * len(mats)
    for m in range(len(mats) - 1, -1, -1):
        deltas[m] = delta
        grads[m] = delta.T @ a[m] / LOSS_SCALE
        back = delta @ mats[m]
        if m > 0:
            d = (a[m] > 0).astype(np.float64) if act == "relu" else 1.0
            delta = _h(back * d, exact)
        else:
            dx = back[:, :n_in] / LOSS_SCALE
    return {"dparams": np.concatenate([gm.ravel() for gm in grads]), "dx": dx, "deltas": deltas, "f": f}
