"""Exact data for tests/test_hashgrid_exact.py: inputs on which every float32 operation of the hash-grid kernels is exact, so
that the HIP encoding must give the float64 oracle (tests/hashgrid_oracle.py) bit for bit, whatever the order of its atomics
and whether or not the compiler fuses a multiply with an add.

With ``per_level_scale = 2.0`` the level scale ``base * 2^l - 1`` is an integer.  ``x`` is a lattice ``k / 2^m``, so ``pos``
and ``frac`` are multiples of ``2^-m``, a corner weight is a multiple of ``2^-3m`` and a weight derivative one of ``2^-2m``;
``params`` are small integers and ``dy`` multiples of ``1 / dy_den``.  Every product and partial sum is then an integer number
of *units* (``2^-3m / dy_den`` for dL/dparams, ``2^-2m / dy_den`` for dL/dx, ``2^-3m`` for the forward), and float32 holds
it exactly while its magnitude stays below 2^24 units.  :func:`conditions` measures exactly that on the oracle; the tests assert
it instead of trusting the recipe.
"""
from __future__ import annotations

import numpy as np

import hashgrid_oracle as O

# lattice name -> (m, lowest k, highest k): x = k / 2^m per axis, reaching below 0 and above 1 (cells that wrap as uint32)
LATTICES = {"scattered": (3, -3, 11), "contended": (1, -1, 3), "coarse": (1, -1, 3)}     # coarse: all 125 points of m = 1
CONTENDED_POINTS = 5                      # "a handful": thousands of adds per entry from N = 16 385 on

CONFIG_A = {"otype": "HashGrid", "n_levels": 5, "n_features_per_level": 2, "log2_hashmap_size": 14, "base_resolution": 4,
            "per_level_scale": 2.0}       # entries 64, 512, 4096 (dense) and 16384, 16384 (hashed)
CONFIG_B = {"otype": "DenseGrid", "n_levels": 4, "n_features_per_level": 2, "base_resolution": 5, "per_level_scale": 2.0}
CONFIG_ONE_LEVEL = dict(CONFIG_A, n_levels=1)
# grid_layout refuses a scale above 65535, so with per_level_scale = 2.0 the deepest config it accepts is base 1 with 17 levels
# (scale 2^16 - 1); 32 levels (the size of the kernels' level table) are reached with per_level_scale = 1.0, which is exact too
CONFIG_17_LEVELS = {"otype": "HashGrid", "n_levels": 17, "n_features_per_level": 2, "log2_hashmap_size": 4, "base_resolution": 1,
                    "per_level_scale": 2.0}
CONFIG_32_LEVELS = {"otype": "HashGrid", "n_levels": 32, "n_features_per_level": 2, "log2_hashmap_size": 4, "base_resolution": 4,
                    "per_level_scale": 1.0}
CONFIG_SECOND_TRIP = dict(CONFIG_A, n_levels=2, n_features_per_level=1)

LDS_BYTES = 128 * 1024                    # csrc/grid.h: kGridLdsBytes (the CPU tier reads the header and compares)


def layout(cfg: dict) -> dict:
    return O.level_layout(cfg["n_levels"], cfg["n_features_per_level"], cfg.get("log2_hashmap_size", 19), cfg["base_resolution"],
                          cfg["per_level_scale"], cfg.get("otype") == "DenseGrid")


def lds_levels(lay: dict, lds_bytes: int = LDS_BYTES) -> int:
    """The prefix of levels whose table (entries x F x 4 bytes) fits in LDS: csrc/grid_capi.cpp's rule, restated."""
    n = 0
    while n < lay["L"] and int(lay["entries"][n]) * lay["F"] * 4 <= lds_bytes:
        n += 1
    return n


def lattice_points(lattice: str, N: int, order: str, seed: int) -> np.ndarray:
    """[N, 3] float32 lattice points, drawn with repetition; order: "random" or "lexsorted" (z slowest, neighbouring rows
    share cells: the on-chip run sums then carry the work)."""
    m, lo, hi = LATTICES[lattice]
    rng = np.random.default_rng(seed)
    if lattice == "contended":
        distinct = rng.permutation((hi - lo + 1) ** 3)[:CONTENDED_POINTS]
        side = hi - lo + 1
        pool = np.stack([distinct % side, distinct // side % side, distinct // (side * side)], 1) + lo
        k = pool[rng.integers(0, CONTENDED_POINTS, N)]
    else:
        k = rng.integers(lo, hi + 1, (N, 3))
    x = (k / float(1 << m)).astype(np.float32)
    if order == "lexsorted":
        x = x[np.lexsort((x[:, 0], x[:, 1], x[:, 2]))]
    else:
        assert order == "random"
    return np.ascontiguousarray(x)


def exact_case(cfg: dict, N: int, lattice: str = "scattered", order: str = "random", seed: int = 0, p_max: int = 4, dy_den: int = 8):
    """(x [N, 3], params [n_params], dy [N, L * F]) as float32: lattice points, integers in [-p_max, p_max], multiples of
    1 / dy_den in [-1, 1]."""
    lay = layout(cfg)
    rng = np.random.default_rng(seed + 1000)
    x = lattice_points(lattice, N, order, seed)
    P = rng.integers(-p_max, p_max + 1, lay["n_params"]).astype(np.float32)
    dy = (rng.integers(-dy_den, dy_den + 1, (N, lay["L"] * lay["F"])) / float(dy_den)).astype(np.float32)
    return x, P, dy


def dx_abs_sum(x: np.ndarray, P: np.ndarray, dy: np.ndarray, lay: dict) -> np.ndarray:
    """[N, 3]: sum_l scale_l sum_c sum_f |v_cf g_f| |d w_c / d pos_d|, the magnitude every partial sum of dL/dx stays below
    (the scale of its float32 rounding error on random data, its exactness condition on exact data)."""
    F, L = lay["F"], lay["L"]
    table = np.abs(np.asarray(P, np.float64)).reshape(-1, F)
    g = np.abs(np.asarray(dy, np.float64))
    out = np.zeros((x.shape[0], 3))
    for l in range(L):
        idx, _, dw = O._corners(x, lay, l)
        s = np.einsum("ncf,nf->nc", table[lay["offset"][l] + idx], g[:, l * F:(l + 1) * F])
        out += np.einsum("nc,ncd->nd", s, np.abs(dw)) * np.float64(lay["scale"][l])
    return out


def _survives_float32(a: np.ndarray) -> bool:
    return bool(np.array_equal(a.astype(np.float32).astype(np.float64), a))


def conditions(x: np.ndarray, P: np.ndarray, dy: np.ndarray, cfg: dict, lattice: str, dy_den: int = 8, prefill: float = 0.0) -> dict:
    """The oracle's results on (x, P, dy) and what makes them the only possible float32 answer: ``survive`` (the oracle's forward,
    dL/dparams and dL/dx are float32 values), and the largest forward, per-entry and per-point-and-axis sums of magnitudes in
    units (each must stay below 2^24).  ``prefill``: the largest magnitude grad_params holds before the backward adds to it."""
    lay = layout(cfg)
    m = LATTICES[lattice][0]
    y = O.encode(x, P, lay)
    gP, gx = O.encode_backward(x, P, dy, lay)
    abs_y = O.encode(x, np.abs(P), lay)
    abs_gP, _ = O.encode_backward(x, P, np.abs(dy), lay)
    abs_gx = dx_abs_sum(x, P, dy, lay)
    return {"y": y, "gP": gP, "gx": gx,
            "survive": _survives_float32(y) and _survives_float32(gP) and _survives_float32(gx),
            "forward_units": float(abs_y.max()) * 2.0 ** (3 * m),
            "entry_units": (float(abs_gP.max()) + prefill) * 2.0 ** (3 * m) * dy_den,
            "dx_units": float(abs_gx.max()) * 2.0 ** (2 * m) * dy_den}


def assert_exact(cond: dict) -> None:
    assert cond["survive"]
    assert cond["forward_units"] < 2 ** 24 and cond["entry_units"] < 2 ** 24 and cond["dx_units"] < 2 ** 24, \
        {k: v for k, v in cond.items() if k.endswith("units")}
