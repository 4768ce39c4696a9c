"""Float64 numpy restatement of the closed-form per-triangle atlas (include/tssplat_amd.h, "texture atlas"): layout, per-wedge
UVs, texel ownership and the baked positions.  Written from the specification alone: it shares no code with
tssplat_amd/atlas.py or csrc/texture_*.

T triangles, a square texture of R texels: n = ceil(sqrt(ceil(T / 2))) cells per row, c = R // n texels per cell, legs of
L = c - 5 texels, c >= 6.  Triangle t sits in cell k = t // 2 with origin ((k % n) c, (k // n) c); even t is half A, odd t
half B.  Texel (i, j) is column i, row j; images are indexed [j, i].
"""
import math

import numpy as np


def layout(T: int, R: int):
    cells = (T + 1) // 2
    n = math.isqrt(cells - 1) + 1                  # ceil(sqrt(ceil(T / 2))) in integers
    assert T >= 1 and (n - 1) ** 2 < cells <= n * n
    c = R // n
    if c < 6:
        raise ValueError(f"smallest workable resolution: {6 * n}")
    return n, c, c - 5


def uv(T: int, R: int):
    """([3 T, 2] float64 texel / R, [T, 3] int32)."""
    n, c, L = layout(T, R)
    out = np.zeros((T, 3, 2))
    for t in range(T):
        k = t // 2
        ox, oy = (k % n) * c, (k // n) * c
        if t % 2 == 0:
            corners = [(1.5, 1.5), (1.5 + L, 1.5), (1.5, 1.5 + L)]
        else:
            corners = [(c - 1.5, c - 1.5), (c - 1.5 - L, c - 1.5), (c - 1.5, c - 1.5 - L)]
        for w, (x, y) in enumerate(corners):
            out[t, w] = (ox + x) / R, (oy + y) / R
    return out.reshape(3 * T, 2), np.arange(3 * T, dtype=np.int32).reshape(T, 3)


def texel_tables(T: int, R: int):
    """owner [R, R] int32 (-1: unowned) and the extrapolated barycentrics b1, b2 [R, R] float64 (0 where unowned)."""
    n, c, L = layout(T, R)
    j, i = np.meshgrid(np.arange(R), np.arange(R), indexing="ij")
    cx, cy = i // c, j // c
    li, lj = i - cx * c, j - cy * c
    inside = (cx < n) & (cy < n)
    k = cy * n + cx
    half_a = inside & (li + lj <= L + 3)
    half_b = inside & (li + lj >= 2 * c - L - 5)
    assert not (half_a & half_b).any()
    owner = np.where(half_a, 2 * k, np.where(half_b, 2 * k + 1, -1))
    owner = np.where(owner >= T, -1, owner)
    b1 = np.where(half_a, (li - 1) / L, (c - 2 - li) / L)
    b2 = np.where(half_a, (lj - 1) / L, (c - 2 - lj) / L)
    own = owner >= 0
    return owner.astype(np.int32), np.where(own, b1, 0.0), np.where(own, b2, 0.0)


def bake(v, tri, R: int):
    """positions [R, R, 3] float64, owner [R, R] int32, b1, b2: a triangle with a vertex index outside [0, nv) is unowned."""
    v, tri = np.asarray(v, np.float64), np.asarray(tri, np.int64)
    owner, b1, b2 = texel_tables(tri.shape[0], R)
    valid = ((tri >= 0) & (tri < v.shape[0])).all(axis=1)
    owner = np.where((owner >= 0) & valid[np.maximum(owner, 0)], owner, -1).astype(np.int32)
    own = owner >= 0
    b1, b2 = np.where(own, b1, 0.0), np.where(own, b2, 0.0)
    t = np.where(valid, 1, 0)[:, None] * tri                      # (invalid triangles: any in-range index, masked below)
    corner = t[np.maximum(owner, 0)]                              # [R, R, 3]
    p = (1.0 - b1 - b2)[..., None] * v[corner[..., 0]] + b1[..., None] * v[corner[..., 1]] + b2[..., None] * v[corner[..., 2]]
    return np.where(own[..., None], p, 0.0), owner, b1, b2


def bilinear_taps(u, v, R: int):
    """The four (i, j, weight) taps of dr.texture's linear filter at uv (float64, no boundary handling)."""
    x, y = u * R - 0.5, v * R - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    return [(x0, y0, (1 - fx) * (1 - fy)), (x0 + 1, y0, fx * (1 - fy)), (x0, y0 + 1, (1 - fx) * fy), (x0 + 1, y0 + 1, fx * fy)]
