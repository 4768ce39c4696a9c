"""Oracle of the colour stage under a blend plan (dr.plan_blends, dr.shade, dr.shade_l1): numpy only, float64, composed of
oracle/raster_oracle.py.

The specification is the operators path of MeshRasterizer.forward(only_alpha=False) -- the point colours scattered into a zero
image, ``lerp`` with the background by the coverage mask, ``antialias`` -- and ``L1Loss`` on the first three channels.  What the
fused kernels rely on is stated here as a second formulation: for a fixed ``rast`` / ``pos`` / ``tri`` the events of
``R.antialias_events`` are data, grouped once by destination (the image) and once by source (the gradient); tests/test_shade.py
asserts on the CPU that the two formulations are the same numbers before any kernel is looked at.

The rounding bounds of the float32 kernels are derived here from their stated operation order (csrc/shade_kernels.hip), the unit
round-off ``EPS = 2^-24``, values in [0, 1] and weights in (0, 1/2]; nothing in them is fitted to an output.
"""
from __future__ import annotations

import numpy as np

import aa_scenes as S
import silhouette_oracle as SO
from oracle import raster_oracle as R

EPS = 2.0 ** -24      # unit round-off of float32
SLACK = 1.0 + 2.0 ** -10   # the second-order terms (1 + EPS)^k - 1 - k EPS of every bound below, generously


# ------------------------------------------------------------------ scenes ------------------------------------------------------------------

def _off_screen(pos):
    """The same vertices moved five screens to the right: projectable, inside the rasteriser's guard band, covering nothing."""
    p = pos.copy()
    p[..., 0] += 10.0 * p[..., 3]
    return p


def _checker_and_sheet(H, W, views):
    return S.merge(SO.sparse_checker(H, W, 27, 3, 6, 47, views=views), S.open_sheet(H, W, views=views, box=(2, -1, 48, 25)))


def _empty_and_covered():
    pos, tri = S.merge(S.checker(20, 36, 3, 4, 5, 9, views=2), S.open_sheet(20, 36, nu=7, nv=6, views=2, box=(14, 2, 34, 18)))
    pos[1] = _off_screen(pos[1])
    return pos, tri


def _nothing_covered():
    pos, tri = S.checker(12, 20, 2, 3, 4, 6, views=2)
    return _off_screen(pos), tri


# name: (builder, (H, W)).  The sizes are the issue's; the last two are small because an empty view is empty at any size.
SCENES = {
    "checker_and_sheet": (lambda: _checker_and_sheet(33, 50, 3), (33, 50)),
    "sparse_checker": (lambda: SO.sparse_checker(24, 160, 9, 10, 6, 140, views=2), (24, 160)),
    "soup": (lambda: S.soup(48, 64), (48, 64)),
    "backdrop_and_sheet": (lambda: S.merge(S.backdrop(32, 32), S.open_sheet(32, 32, nu=9, nv=8, views=1)), (32, 32)),
    "empty_and_covered": (_empty_and_covered, (20, 36)),
    "nothing_covered": (_nothing_covered, (12, 20)),
}
FOUR_CHANNEL_TARGET = {"sparse_checker", "backdrop_and_sheet", "nothing_covered"}      # half of the cases


def inputs(scene, n_points, shape, seed=11):
    """(color[N, 3], background[B, H, W, 3], target[B, H, W, 3 or 4]) float32, uniform in [0, 1)."""
    rng = np.random.default_rng([seed, sorted(SCENES).index(scene)])
    color = rng.random((n_points, 3), dtype=np.float32)
    background = rng.random(tuple(shape) + (3,), dtype=np.float32)
    target = rng.random(tuple(shape) + (4 if scene in FOUR_CHANNEL_TARGET else 3,), dtype=np.float32)
    return color, background, target


# ------------------------------------------------------------------ the plan ------------------------------------------------------------------

def pix_point(rast):
    """``int32[B * H * W]``: the exclusive prefix count of ``rast[..., 3] > 0`` on foreground (the row of the pixel in
    ``positions_all[selector]``), -1 on background; and the number of points."""
    fg = (np.asarray(rast)[..., 3] > 0).reshape(-1)
    rank = np.cumsum(fg) - 1
    return np.where(fg, rank, -1).astype(np.int32), int(fg.sum())


def records(events, H, W):
    """The events of ``R.antialias_events`` as ``(dst, src, weight)`` arrays, pixel indices batch-wide, in the oracle's order;
    ``weight`` is the oracle's float64."""
    dst, src, wgt = [], [], []
    for b, evs in enumerate(events):
        for ev in evs:
            dst.append((b * H + ev[0][0]) * W + ev[0][1])
            src.append((b * H + ev[1][0]) * W + ev[1][1])
            wgt.append(ev[2])
    return np.asarray(dst, dtype=np.int64), np.asarray(src, dtype=np.int64), np.asarray(wgt, dtype=np.float64)


def csr(keys):
    """Stable grouping: ``(perm, group keys, ptr)`` with the records of group ``s`` at ``perm[ptr[s]:ptr[s + 1]]`` in their
    original order."""
    perm = np.argsort(keys, kind="stable")
    group, counts = np.unique(keys[perm], return_counts=True)
    return perm, group, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def most_per_group(keys):
    return int(np.unique(keys, return_counts=True)[1].max()) if len(keys) else 0


# ------------------------------------------------------------------ image, loss, gradient ------------------------------------------------------------------

def lerp(a, b, w):
    """torch.lerp's two-sided formula: exact at w = 0 and w = 1."""
    return np.where(w < 0.5, a + w * (b - a), b - (b - a) * (1.0 - w))


def composite(color, background, rast):
    """``lerp(background, scatter(color), mask)`` of the operators path, ``[B, H, W, 3]`` float64."""
    mask = np.asarray(rast)[..., 3] > 0
    fg = np.zeros(mask.shape + (3,))
    fg[mask] = np.asarray(color, dtype=np.float32).astype(np.float64)
    return lerp(np.asarray(background, dtype=np.float32).astype(np.float64), fg, mask[..., None].astype(np.float64))


def shade_operators(color, background, rast, pos, tri, events):
    """The specification: ``R.antialias`` of the composite."""
    return R.antialias(composite(color, background, rast).astype(np.float32), rast, pos, tri, events=events)


def shade_csr(color, background, rast, dst, src, wgt):
    """The plan's formulation: ``c_p`` from ``pix_point``, then per destination its records in order."""
    pp, _ = pix_point(rast)
    bg = np.asarray(background, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    col = np.asarray(color, dtype=np.float32).astype(np.float64)
    c = np.where((pp >= 0)[:, None], col[np.maximum(pp, 0)] if len(col) else bg, bg)
    out = c.copy()
    perm, group, ptr = csr(dst)
    for s, p in enumerate(group):
        for r in perm[ptr[s]:ptr[s + 1]]:
            out[p] += wgt[r] * (c[src[r]] - c[p])
    return out.reshape(np.asarray(background).shape)


def l1(image, target):
    """float64 ``L1Loss`` of the first three channels."""
    d = np.asarray(image, dtype=np.float64)[..., :3] - np.asarray(target, dtype=np.float32).astype(np.float64)[..., :3]
    return float(np.mean(np.abs(d))) if d.size else 0.0


def l1_grad(image, target, upstream=1.0):
    """d (upstream * l1) / d image = sign(image - target) upstream / n with sign(0) = 0, ``[B, H, W, 3]``."""
    d = np.asarray(image, dtype=np.float64)[..., :3] - np.asarray(target, dtype=np.float32).astype(np.float64)[..., :3]
    return np.sign(d) * float(upstream) / max(d.size, 1)


def grad_color_csr(g, rast, dst, src, wgt):
    """The transposed form: ``grad_color[k] = g_p (1 - sum_{dst = p} w) + sum_{src = p} w g_dst`` for the pixel p of point k."""
    pp, n_points = pix_point(rast)
    g = np.asarray(g, dtype=np.float64).reshape(-1, 3)
    keep = np.ones(len(pp))
    np.subtract.at(keep, dst, wgt)
    full = g * keep[:, None]
    np.add.at(full, src, wgt[:, None] * g[dst])
    return full[pp >= 0].reshape(n_points, 3)


def grad_color_operators(g, color, background, rast, pos, tri, events):
    """The specification: ``R.antialias_backward`` w.r.t. the composite, gathered at the foreground pixels."""
    gc, _ = R.antialias_backward(composite(color, background, rast).astype(np.float32), rast, pos, tri, g, events=events)
    return gc[np.asarray(rast)[..., 3] > 0]


# ------------------------------------------------------------------ rounding bounds ------------------------------------------------------------------

def image_bound(K):
    """|out32 - out64| per element for a destination with at most K records, inputs in [0, 1], weights w in (0, 1/2].

    The kernel computes ``out = c;  out = fl(out + fl(w32 * fl(c_src - c)))`` per record.  Per record: the weight is the oracle's
    float64 rounded once (|w32 - w| <= EPS / 2, times |c_src - c| <= 1), the difference and the product round once each
    (relative 2 EPS of a term of at most 1/2): 3/2 EPS.  Every partial sum is at most 1 + K / 2 in magnitude and rounds once:
    K (1 + K / 2) EPS.  Without records out = c exactly."""
    return (1.5 * K + K * (1.0 + 0.5 * K)) * EPS * SLACK


def loss_bound(K):
    """|loss32 - l1(out64, target)|: a mean of terms ``|fl(out32 - t)|`` each within ``image_bound(K)`` plus one rounding of a
    difference of at most 2 + K / 2, accumulated in float64 (~1e-16, absorbed in SLACK), and one final rounding to float32 of a
    value of at most 2 + K / 2."""
    return image_bound(K) + 2.0 * (2.0 + 0.5 * K) * EPS * SLACK


def grad_bound(Kd, Ks, G):
    """|grad_color32 - grad_color64| per element where every g has magnitude G = upstream / n (or 0): at most Kd records on the
    point's own pixel as a destination and Ks with it as the source.

    The kernel computes ``a = ((w_0 + w_1) + ...)``, ``acc = fl(g_p * fl(1 - a))``, then ``acc = fl(acc + fl(w * g_dst))`` per source
    record, with ``g = sign * fl(upstream / n)`` (one rounding, relative EPS, in every term).  a: Kd weights rounded once (EPS / 2
    each) and Kd - 1 sums of at most Kd / 2: Kd / 2 + Kd^2 / 2.  1 - a and its product with g: two roundings of at most 1 + Kd / 2,
    and g's own: 3 (1 + Kd / 2).  Per source record weight, g and product round once on a term of at most G / 2: 3 / 2; the Ks
    partial sums are at most 1 + Kd / 2 + Ks / 2."""
    units = 0.5 * Kd + 0.5 * Kd * Kd + 3.0 * (1.0 + 0.5 * Kd) + 1.5 * Ks + Ks * (1.0 + 0.5 * Kd + 0.5 * Ks)
    return units * EPS * SLACK * abs(G)
