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

Also here: ``plan`` (which kernel variant, pass split and LDS mode the launch code picks for a config) and
``dense_exact_data`` / ``exact_preconditions`` (integer data on which the kernels' arithmetic is exact and dW is dense).
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


def _image_halfs(rows: int, cols: int) -> int:
    """fp16 elements of the A-operand fragment image of a [rows, cols] matrix: 16-row tiles x 32-wide k-steps x 64 lanes x 8."""
    return (rows // 16) * ((cols + 31) // 32) * 64 * 8


def plan(n_in: int, n_out: int, width: int, n_hidden: int) -> dict:
    """What launch_mlp_forward / launch_mlp_backward choose for a config, restated from the comments and constants of
    csrc/mlp.h and csrc/mlp_kernels.hip (kMlpResidentBytes = 64 KiB, kMlpImageStride = 72, four waves per workgroup):

    * ``tiles``: 16 x 16 dW tiles per matrix; ``slots``: 8 tiles per wave when they sum to at most 32, else 32 (the
      mlp_backward_kernel<W, SLOTS> instantiation); ``cap``: at most 512 (slots 8) or 256 workgroups;
    * ``passes``: (lo, hi) groups of consecutive matrices whose tiles fit 4 x slots, one backward launch each;
    * ``fwd_resident`` / ``bwd_resident``: the fragment images (the backward: plus their transposes') fit 64 KiB;
    * ``fwd_lds`` / ``bwd_lds``: dynamic LDS bytes; the backward adds the [neuron][row] delta and input images;
    * ``cls``: (width, slots, multi-pass, forward resident, backward resident, backward LDS above 64 KiB)."""
    lay = layout(n_in, n_out, width, n_hidden)
    shapes = lay["shapes"]
    tiles = [(r // 16) * (c // 16) for r, c in shapes]
    slots = 8 if sum(tiles) <= 32 else 32
    passes, lo = [], 0
    while lo < len(tiles):
        hi, used = lo - 1, 0
        while hi + 1 < len(tiles) and used + tiles[hi + 1] <= 4 * slots:
            hi += 1
            used += tiles[hi]
        passes.append((lo, hi))
        if hi < lo:                                                    # a matrix that fits no pass: reported, not looped on
            break
        lo = hi + 1
    fwd = [_image_halfs(r, c) for r, c in shapes]
    tr = [_image_halfs(c, r) for r, c in shapes]
    fwd_resident = 2 * sum(fwd) <= 64 * 1024
    bwd_resident = 2 * (sum(fwd) + sum(tr)) <= 64 * 1024
    images = (max(lay["out_w"], width) + max(lay["in_w"], width)) * 72
    bwd_lds = 2 * ((sum(fwd) + sum(tr) if bwd_resident else max(fwd + tr)) + images)
    return {"tiles": tiles, "slots": slots, "cap": 512 if slots == 8 else 256, "passes": passes, "fwd_resident": fwd_resident,
            "bwd_resident": bwd_resident, "fwd_lds": 2 * (sum(fwd) if fwd_resident else max(fwd)), "bwd_lds": bwd_lds,
            "cls": (width, slots, len(passes) > 1, fwd_resident, bwd_resident, bwd_lds > 64 * 1024)}


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


def _tiled_permutation(rng, rows: int, cols: int, fan: int) -> np.ndarray:
    """[rows, fan] column indices drawn from concatenated permutations of range(cols): every column is hit once rows * fan
    >= cols, and no column more than ceil(rows * fan / cols) times."""
    n = rows * fan
    return np.concatenate([rng.permutation(cols) for _ in range((n + cols - 1) // cols)])[:n].reshape(rows, fan)


def dense_exact_data(n_in, n_out, width, n_hidden, N, seed, out_scale=1.0):
    """(x, params, dy) on which the kernels' fp16 / fp32 arithmetic is exact and dW is dense (`exact_preconditions` asserts
    both).  Every hidden matrix is the sum of two tiled permutations, one with entries +1 (ReLU networks stay alive), one with
    random +-1 (a -1 that lands on a +1 is flipped, so no entry cancels), no row dropped; the first matrix takes
    ceil(in_w / W) entries per row and permutation, so that every input column reaches some neuron and dx has no dead column.
    The output matrix is dense +-1 times ``out_scale`` (a power of two).  x is integer in [-2, 2], dy = k / 128 with |k| <= 2."""
    rng = np.random.default_rng(seed)
    lay = layout(n_in, n_out, width, n_hidden)
    parts = []
    for m, (rows, cols) in enumerate(lay["shapes"]):
        if m == n_hidden:
            mat = rng.choice([-1.0, 1.0], (rows, cols)) * out_scale
        else:
            one, signed = np.zeros((rows, cols)), np.zeros((rows, cols))
            fan = (cols + rows - 1) // rows
            r = np.repeat(np.arange(rows), fan)
            np.add.at(one, (r, _tiled_permutation(rng, rows, cols, fan).ravel()), 1.0)
            np.add.at(signed, (r, _tiled_permutation(rng, rows, cols, fan).ravel()), rng.choice([-1.0, 1.0], rows * fan))
            signed[(one != 0) & (one + signed == 0)] *= -1.0           # a -1 that would cancel a +1 becomes +1: no column dies
            mat = one + signed
        parts.append(mat.ravel())
    x = rng.integers(-2, 3, (N, n_in)).astype(np.float64)
    dy = rng.integers(-2, 3, (N, n_out)) / 128.0
    return x, np.concatenate(parts), dy


def exact_preconditions(x, params, dy, n_out, width, n_hidden, act="relu", out_act="none", dense=True) -> dict:
    """Asserts what makes `dense_exact_data` a bitwise known answer and a dense one, and returns the exact-mode backward:

    * the rounding mode equals the exact mode for y, dx and dparams (every fp16 rounding is the identity);
    * every |a| and |S delta| is at most 2048 (the integers fp16 holds exactly);
    * sum over rows of |S delta| |a| stays below 2^24 for every dW entry, so any fp32 summation order is exact;
    * no 16 x 16 dW tile over real output rows is all zero, at least a quarter of dW is non-zero, every padded output row of
      dW is exactly zero, and every real input column of dx is non-zero in some row.

    ``dense=False`` (a single row, which cannot fill a matrix) keeps the exactness conditions and the zero padded rows only.
    The returned dict adds ``stats``: the figures themselves."""
    ex = backward(x, params, dy, n_out, width, n_hidden, act, out_act, exact=True)
    rd = backward(x, params, dy, n_out, width, n_hidden, act, out_act, exact=False)
    assert np.array_equal(ex["f"]["y"], rd["f"]["y"]) and np.array_equal(ex["dx"], rd["dx"])
    assert np.array_equal(ex["dparams"], rd["dparams"])
    lay = ex["f"]["lay"]
    biggest = max(float(np.abs(v).max()) for v in ex["f"]["a"] + ex["deltas"])
    assert biggest <= 2048, biggest
    mass, tile_share, off = 0.0, 1.0, 0
    for m, (rows, cols) in enumerate(lay["shapes"]):
        mass = max(mass, float((np.abs(ex["deltas"][m]).T @ np.abs(ex["f"]["a"][m])).max()))
        g = ex["dparams"][off:off + rows * cols].reshape(rows, cols)
        off += rows * cols
        real = n_out if m == n_hidden else rows
        assert not g[real:].any(), m                                   # padded output rows
        for rt in range((real + 15) // 16):
            for ct in range(cols // 16):
                tile = g[16 * rt:min(16 * rt + 16, real), 16 * ct:16 * ct + 16]
                tile_share = min(tile_share, float(np.count_nonzero(tile)) / tile.size)
    assert mass < 2.0 ** 24, mass
    share = float(np.count_nonzero(ex["dparams"])) / ex["dparams"].size
    if dense:
        assert tile_share > 0.0
        assert share >= 0.25, share
        assert np.abs(ex["dx"]).max(axis=0).min() > 0.0
    ex["stats"] = {"max_value": biggest, "dw_mass": mass, "dw_share": share, "sparsest_tile": tile_share,
                   "dx_share": float(np.count_nonzero(ex["dx"])) / ex["dx"].size}
    return ex
