"""Scenes for the antialias parity tests (tests/test_antialias_edges.py): numpy only, no GPU, no pytest.

Every builder returns ``(pos[B, V, 4] float32, tri[T, 3] int32)``: clip-space positions made directly from pixel coordinates
(``x = px / W * 2 - 1``, ``y = py / H * 2 - 1``, ``w = 1`` unless stated) and one triangle list shared by the views.  The views
of one scene differ (a small shift, other depths), so that a kernel reading another view's positions, windows or flags shows.

The second half of the file reads a ``rast`` image the way the antialias kernels do -- which pixel pairs differ, which triangle
wins a pair -- so that a test can assert, on the image it is about to use, that the scene still produces its case.
"""
from __future__ import annotations

import numpy as np


def _clip(px, py, z, H, W):
    """Clip-space rows (w = 1) of points given in pixels."""
    px, py, z = np.broadcast_arrays(np.asarray(px, dtype=np.float64), np.asarray(py, dtype=np.float64), np.asarray(z, dtype=np.float64))
    return np.stack([px / W * 2.0 - 1.0, py / H * 2.0 - 1.0, z, np.ones_like(px)], axis=-1)


def _quads(x0, y0, x1, y1, z, H, W):
    """Separate quads ``[x0, x1] x [y0, y1]`` (arrays of n), own four vertices each, split along the diagonal that does NOT pass
    through a pixel centre 0.2 pixel inside the lower left corner: ``pos[4 n, 4]``, ``tri[2 n, 3]``."""
    n = len(x0)
    px = np.stack([x0, x1, x1, x0], axis=1)
    py = np.stack([y0, y0, y1, y1], axis=1)
    pos = _clip(px, py, np.asarray(z)[:, None], H, W).reshape(4 * n, 4)
    base = 4 * np.arange(n)[:, None]
    tri = np.concatenate([base + [0, 1, 3], base + [1, 2, 3]], axis=1).reshape(2 * n, 3)
    return pos, tri


def merge(*scenes):
    """One scene out of several with the same number of views: vertices concatenated, triangle lists renumbered."""
    pos, tri, v = [], [], 0
    for p, t in scenes:
        pos.append(p)
        tri.append(t + v)
        v += p.shape[1]
    return np.concatenate(pos, axis=1).astype(np.float32), np.concatenate(tri).astype(np.int32)


def backdrop(H, W, views=1, z=0.9):
    """Two triangles over the whole image, behind everything else."""
    pos = _clip([-1.0, W + 1.0, W + 1.0, -1.0], [-1.0, -1.0, H + 1.0, H + 1.0], z, H, W)
    return np.repeat(pos[None], views, axis=0).astype(np.float32), np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)


def checker(H, W, j0, i0, nj, ni, off=(0.3, 0.3), views=1, seed=0):
    """``nj x ni`` separate unit-pixel quads from pixel ``(j0, i0)`` on, shifted by ``off`` pixels, a random depth per quad and
    view: every pixel of the block shows another triangle than its neighbours (a pair on both axes: 128 pairs per full 64-pixel
    chunk), every outer edge of a quad is a boundary edge (``opp = -1``), its diagonal has a partner.  View ``b`` is shifted by a
    further ``0.07 b`` pixels."""
    rng = np.random.default_rng(seed)
    jj, ii = (a.reshape(-1).astype(np.float64) for a in np.meshgrid(np.arange(nj), np.arange(ni), indexing="ij"))
    pos = []
    for b in range(views):
        x0, y0 = i0 + ii + off[0] + 0.07 * b, j0 + jj + off[1] + 0.07 * b
        p, tri = _quads(x0, y0, x0 + 1.0, y0 + 1.0, rng.uniform(-0.5, 0.5, nj * ni), H, W)
        pos.append(p)
    return np.stack(pos).astype(np.float32), tri.astype(np.int32)


def comb(H, W, j0, i0, length, n, axis, off=0.3, views=1, seed=0):
    """``n`` separate strips, one pixel wide and ``length`` pixels long, side by side: vertical strips for ``axis == 0`` (their
    long edges make horizontal pairs in every row), horizontal strips for ``axis == 1``.  Four vertices per strip take the
    ``grad_pos`` contributions of ``~ length`` pairs each."""
    rng = np.random.default_rng(seed)
    k = np.arange(n, dtype=np.float64)
    pos = []
    for b in range(views):
        s = off + 0.07 * b
        if axis == 0:
            x0, y0 = i0 + k + s, np.full(n, j0 + s)
            x1, y1 = x0 + 1.0, y0 + length
        else:
            x0, y0 = np.full(n, i0 + s), j0 + k + s
            x1, y1 = x0 + length, y0 + 1.0
        p, tri = _quads(x0, y0, x1, y1, rng.uniform(-0.5, 0.5, n), H, W)
        pos.append(p)
    return np.stack(pos).astype(np.float32), tri.astype(np.int32)


def open_sheet(H, W, nu=12, nv=10, views=1, box=None, seed=0):
    """A regular triangulated patch (``nu x nv`` vertices, open boundary all round) over the pixel box ``(x0, y0, x1, y1)``
    (default: the image with a 3-pixel margin), folded into an S along x so that three layers overlap in the middle: boundary
    edges all round and fold lines -- silhouette edges WITH a partner -- inside."""
    rng = np.random.default_rng(seed)
    x0, y0, x1, y1 = box if box is not None else (3.0, 3.0, W - 3.0, H - 3.0)
    u, v = np.meshgrid(np.linspace(0.0, 1.0, nu), np.linspace(0.0, 1.0, nv), indexing="xy")        # [nv, nu]
    pos = []
    for b in range(views):
        fold = 0.30 + 0.02 * b
        s = (u + fold * np.sin(3.0 * np.pi * u)) / 1.0                                             # d s / d u < 0 in two bands: folds
        s = (s - s.min()) / (s.max() - s.min())
        px = x0 + (x1 - x0) * s + 0.37 * np.sin(5.0 * v + b)
        py = y0 + (y1 - y0) * (v + 0.04 * np.sin(4.0 * u + 0.5 * b))
        z = 0.6 * (u - 0.5) + 0.15 * np.sin(3.0 * v) + 0.01 * rng.standard_normal(u.shape)
        pos.append(_clip(px, py, z, H, W).reshape(nu * nv, 4))
    k = (np.arange(nv - 1)[:, None] * nu + np.arange(nu - 1)[None, :]).reshape(-1, 1)
    tri = np.concatenate([k + [0, 1, nu], k + [1, nu + 1, nu]], axis=1).reshape(-1, 3)
    return np.stack(pos).astype(np.float32), tri.astype(np.int32)


SOUP_BEHIND = (5, 17)       # vertices at w <= 0
SOUP_NAN = 9                # NaN x
SOUP_FAR = 23               # beyond the rasteriser's guard band (but projectable: antialias reads it as a far-away point)
SOUP_FAN = (30, 31)         # an edge shared by three triangles


def soup(H, W, n_vertices=40, n_tri=120, seed=3):
    """A random triangle soup over ``n_vertices`` vertices at eighth-of-the-screen positions with ``w`` in [0.5, 3): shared edges
    through pixel centres, an edge with three triangles (``SOUP_FAN``), ten duplicate triangles, a degenerate one; vertices
    ``SOUP_BEHIND`` at ``w <= 0``, ``SOUP_NAN`` with a NaN x, ``SOUP_FAR`` beyond the guard band.  Two views: the second is the
    first with the vertex order reversed (the same triangle list then names other points)."""
    rng = np.random.default_rng(seed)
    pts = np.round(rng.uniform(-1.2, 1.2, (n_vertices, 2)) * 8) / 8
    w = rng.uniform(0.5, 3.0, n_vertices)
    pos = np.concatenate([pts * w[:, None], (rng.uniform(-0.9, 0.9, n_vertices) * w)[:, None], w[:, None]], axis=1).astype(np.float32)
    pos[SOUP_BEHIND[0], 3] = -0.5
    pos[SOUP_BEHIND[1], 3] = 0.0
    pos[SOUP_NAN, 0] = np.nan
    pos[SOUP_FAR, 0] = 2.0 * 20000.0 / W * pos[SOUP_FAR, 3]
    tri = rng.integers(0, n_vertices, (n_tri, 3))
    a, b = SOUP_FAN
    tri = np.concatenate([tri, [[a, b, 2], [a, b, 12], [b, a, 33]], tri[:10], [[1, 1, 2]]])
    return np.stack([pos, pos[::-1].copy()]).astype(np.float32), tri.astype(np.int32)


# ------------------------------------------------ reading a rast image like the kernels do ------------------------------------------------

def differing_pairs(rast):
    """``c[B, H, W, 2]``: pixel ``(j, i)`` shows another triangle id than its right (axis 0) / upper (axis 1) neighbour."""
    ids = np.asarray(rast)[..., 3]
    c = np.zeros(ids.shape + (2,), dtype=bool)
    c[:, :, :-1, 0] = ids[:, :, 1:] != ids[:, :, :-1]
    c[:, :-1, :, 1] = ids[:, 1:, :] != ids[:, :-1, :]
    return c


def pairs_per_chunk(rast):
    """Pairs (both axes) per 64 consecutive pixels of the whole batch, the last chunk padded: what one mask chunk holds."""
    c = differing_pairs(rast).reshape(-1, 2).sum(axis=1)
    n = (len(c) + 63) // 64
    return np.concatenate([c, np.zeros(n * 64 - len(c), dtype=c.dtype)]).reshape(n, 64).sum(axis=1)


def pair_winners(rast_b):
    """For one view: the pairs as ``(j, i, axis)`` rows and the triangle id that wins each (the closer of the two, ties to the
    second pixel, background never) -- the oracle's choice, restated only to COUNT pairs by the kind of their triangle."""
    rast_b = np.asarray(rast_b)
    ids = rast_b[..., 3].astype(np.int64) - 1
    zw = rast_b[..., 2]
    rows, win = [], []
    for axis, (dj, di) in enumerate(((0, 1), (1, 0))):
        H, W = ids.shape
        t0, t1 = ids[:H - dj, :W - di], ids[dj:, di:]
        z0, z1 = zw[:H - dj, :W - di], zw[dj:, di:]
        jj, ii = np.nonzero(t0 != t1)
        a0, a1 = t0[jj, ii], t1[jj, ii]
        first = np.where((a0 >= 0) & (a1 >= 0), z0[jj, ii] < z1[jj, ii], a0 >= 0)
        rows.append(np.stack([jj, ii, np.full_like(jj, axis)], axis=1))
        win.append(np.where(first, a0, a1))
    return np.concatenate(rows), np.concatenate(win)


def projectable(pos_b):
    """Per vertex of one view: antialias can project it (finite x, y, w and w > 0)."""
    p = np.asarray(pos_b, dtype=np.float64)
    return np.isfinite(p[:, [0, 1, 3]]).all(axis=1) & (p[:, 3] > 0.0)


def edge_slots(tri):
    """``{(lo, hi): [3 t + e, ...]}``: the (triangle, edge) slots on every undirected vertex pair -- one for a boundary edge, two
    for a manifold edge, more for a non-manifold one."""
    slots = {}
    for t, row in enumerate(np.asarray(tri).reshape(-1, 3).tolist()):
        for e in range(3):
            a, b = row[(e + 1) % 3], row[(e + 2) % 3]
            slots.setdefault((min(a, b), max(a, b)), []).append(3 * t + e)
    return slots


def dense_aligned_runs(per_chunk, group, at_least=100):
    """Number of group-aligned runs of ``group`` chunks (one wave's share) in which EVERY chunk holds ``at_least`` pairs, and the
    largest pair count of such a run."""
    n = len(per_chunk) // group * group
    runs = np.asarray(per_chunk[:n]).reshape(-1, group)
    dense = (runs >= at_least).all(axis=1)
    return int(dense.sum()), int(runs[dense].sum(axis=1).max()) if dense.any() else 0
