"""Float64 numpy oracle of the multiresolution hash-grid encoding (tssplat_amd/encoding.py, csrc/grid_kernels.hip).

The encoding is Instant-NGP's (Mueller, Evans, Schied, Keller, "Instant Neural Graphics Primitives with a Multiresolution
Hash Encoding", SIGGRAPH 2022) as tiny-cuda-nn's ``Grid`` encoding implements it (its published ``encodings/grid.h``:
``grid_scale`` / ``grid_resolution`` / ``grid_index`` / ``kernel_grid``), restated rule by rule:

* level scale and resolution, both in FLOAT32 and in this order:
  ``scale_l = exp2f(l * log2f(per_level_scale)) * base_resolution - 1``, ``res_l = ceil(scale_l) + 1``, with exp2f / log2f
  correctly rounded (libm's and the device's may differ in the last ulp; here both are evaluated in float64 and rounded)
  (float64 arithmetic can give a different grid: see ``test_hashgrid.py::test_layout_float32_boundary``);
* entries per level ``min(next_multiple(res_l^3, 8), 2^log2_hashmap_size)`` for ``Hash`` (no cap for ``Dense``), levels laid
  out one after another, each entry ``n_features_per_level`` contiguous values;
* cell ``pos = fmaf(scale_l, x, 0.5f)``, ``cell = (uint32)(int)floorf(pos)``, ``frac = pos - floorf(pos)``; inputs are NOT
  clamped and a negative cell wraps as uint32;
* index: the dense stride index ``x + y res + z res^2`` while the stride stays <= the level's entry count, else (``Hash``) the
  coherent prime hash ``x * 1 ^ y * 2654435761 ^ z * 805459861``, uint32 wrap-around, either taken ``% entries``;
* trilinear interpolation; output ``[N, L * F]``, level-major columns;
* backward: ``dL/dparams`` = interpolation weight x ``dL/dy`` scattered; ``dL/dx = sum_l sum_f dL/dy * d interp / d pos * scale_l``.

PARITY UNPINNED: tiny-cuda-nn is a CUDA-only library and cannot run here, so bit parity with the library itself is not
checked; this file is the definition the HIP kernels are tested against.  The cell position is formed in float32 exactly as
above (it decides the cell); interpolation and gradients are float64.

DOMAIN: finite ``x`` with ``|scale_l * x + 0.5| < 2^31`` on every level.  Outside it (larger positions, +-inf, NaN) this file
and the kernels disagree by construction -- the integer conversion wraps here and saturates on the device -- and the values
of such rows (their outputs, their dL/dx and what they add to dL/dparams) are unspecified.  Every table index is still reduced
modulo the level's entry count, so all accesses stay in bounds, and the other rows' outputs and dL/dx are not affected
(tests/test_hashgrid_exact.py pins that).
"""
from __future__ import annotations

import math

import numpy as np

PRIMES = (1, 2654435761, 805459861)
_M32 = np.uint64(0xFFFFFFFF)


def _next_multiple(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def level_layout(n_levels: int, n_features_per_level: int, log2_hashmap_size: int, base_resolution: int,
                 per_level_scale: float, dense: bool = False) -> dict:
    """Per-level ``scale`` (float32), ``res``, ``entries``, ``offset`` (in entries), ``is_hash`` and ``n_params``."""
    # log2f / exp2f correctly rounded: evaluated in float64 and rounded to float32 (tsamd_grid_layout does the same)
    log2_scale = np.float32(np.log2(np.float64(np.float32(per_level_scale))))
    T = 1 << log2_hashmap_size
    scales, res, entries, offsets, is_hash = [], [], [], [], []
    off = 0
    for l in range(n_levels):
        s = np.float32(np.float32(np.exp2(np.float64(np.float32(l) * log2_scale))) * np.float32(base_resolution) - np.float32(1.0))
        r = int(math.ceil(float(s))) + 1
        n = _next_multiple(r ** 3, 8)
        if not dense:
            n = min(n, T)
        # grid_index: the stride loop runs in uint32 while stride <= entries; hashed when the stride passed the entries
        stride = 1
        for _ in range(3):
            if stride > n:
                break
            stride = (stride * r) & 0xFFFFFFFF
        scales.append(s)
        res.append(r)
        entries.append(n)
        offsets.append(off)
        is_hash.append((not dense) and n < stride)
        off += n
    return {"scale": np.array(scales, np.float32), "res": np.array(res, np.int64), "entries": np.array(entries, np.int64),
            "offset": np.array(offsets + [off], np.int64), "is_hash": np.array(is_hash, bool),
            "n_params": off * n_features_per_level, "F": n_features_per_level, "L": n_levels}


def cell_position(x: np.ndarray, scale: np.float32, exact: bool = False):
    """``fmaf(scale, x, 0.5f)`` (the float64 product of two float32 values is exact), its uint32 cell and frac.
    exact=True keeps x and pos in float64 (for finite differences in x)."""
    if exact:
        pos = np.float64(scale) * np.asarray(x, np.float64) + 0.5
    else:
        pos = (np.float64(scale) * x.astype(np.float32).astype(np.float64) + 0.5).astype(np.float32)
    fl = np.floor(pos)
    cell = fl.astype(np.int64).astype(np.uint64) & _M32
    return cell, (pos - fl).astype(np.float64)


def grid_index(corner: np.ndarray, res: int, entries: int, is_hash: bool) -> np.ndarray:
    """corner: uint64 [..., 3] holding uint32 values."""
    c = corner.astype(np.uint64) & _M32
    if is_hash:
        h = np.zeros(c.shape[:-1], np.uint64)
        for d in range(3):
            h ^= (c[..., d] * np.uint64(PRIMES[d])) & _M32
        idx = h
    else:
        r = np.uint64(res)
        idx = (c[..., 0] + c[..., 1] * r + ((c[..., 2] * ((r * r) & _M32)) & _M32)) & _M32
    return (idx % np.uint64(entries)).astype(np.int64)


def _corners(x: np.ndarray, lay: dict, l: int, exact: bool = False):
    """The 8 corners of every point at level l: (entry index [N, 8], weights [N, 8], dweights/dpos [N, 8, 3])."""
    cell, frac = cell_position(x, lay["scale"][l], exact)
    N = x.shape[0]
    idx = np.empty((N, 8), np.int64)
    w = np.empty((N, 8))
    dw = np.empty((N, 8, 3))
    for c in range(8):
        bits = [(c >> d) & 1 for d in range(3)]
        corner = cell + np.array(bits, np.uint64)
        idx[:, c] = grid_index(corner, int(lay["res"][l]), int(lay["entries"][l]), bool(lay["is_hash"][l]))
        f = [frac[:, d] if bits[d] else 1.0 - frac[:, d] for d in range(3)]
        w[:, c] = f[0] * f[1] * f[2]
        for d in range(3):
            s = 1.0 if bits[d] else -1.0
            o = [f[e] for e in range(3) if e != d]
            dw[:, c, d] = s * o[0] * o[1]
    return idx, w, dw


def encode(x: np.ndarray, params: np.ndarray, lay: dict, exact: bool = False) -> np.ndarray:
    """Forward: [N, 3] -> [N, L * F] (float64)."""
    F, L = lay["F"], lay["L"]
    P = np.asarray(params, np.float64).reshape(-1, F)
    out = np.empty((x.shape[0], L * F))
    for l in range(L):
        idx, w, _ = _corners(x, lay, l, exact)
        vals = P[lay["offset"][l] + idx]                       # [N, 8, F]
        out[:, l * F:(l + 1) * F] = np.einsum("nc,ncf->nf", w, vals)
    return out


def encode_backward(x: np.ndarray, params: np.ndarray, dy: np.ndarray, lay: dict, exact: bool = False):
    """(dL/dparams [n_params], dL/dx [N, 3]) for the upstream gradient dy [N, L * F] (float64)."""
    F, L = lay["F"], lay["L"]
    P = np.asarray(params, np.float64).reshape(-1, F)
    dy = np.asarray(dy, np.float64)
    gP = np.zeros_like(P)
    gx = np.zeros((x.shape[0], 3))
    for l in range(L):
        idx, w, dw = _corners(x, lay, l, exact)
        g = dy[:, l * F:(l + 1) * F]                           # [N, F]
        rows = lay["offset"][l] + idx
        for f in range(F):
            gP[:, f] += np.bincount(rows.reshape(-1), weights=(w * g[:, None, f]).reshape(-1), minlength=gP.shape[0])
        s = np.einsum("ncf,nf->nc", P[rows], g)                 # dL/d(corner weight)
        gx += np.einsum("nc,ncd->nd", s, dw) * np.float64(lay["scale"][l])
    return gP.reshape(-1), gx
