"""The exact point-to-triangle search in numpy -- TEST INFRASTRUCTURE, the statement ``tssplat_amd.metrics.nearest_on_mesh`` is held to.

Valid triangles.  A triangle is valid iff its three indices lie in ``[0, V)``, its nine coordinates are finite and the sampler's
float64 weight ``w`` (``metrics_oracle.face_normals``: the cross product as two rounded products and a difference per component,
``w = sqrt((nx nx + ny ny) + nz nz)``) is ``> 0``.  An invalid triangle is never a result and nothing is read through a bad index.

Distance per pair (query ``P``, valid triangle ``A B C``): float64 on the float32 inputs, every operation rounded on its own, the
Voronoi-region method of Ericson, Real-Time Collision Detection, section 5.1.5.  With ``dot(u, v) = (ux vx + uy vy) + uz vz``::

    AB = B - A, AC = C - A, AP = P - A, BP = P - B, CP = P - C
    d1 = dot(AB, AP)  d2 = dot(AC, AP)  d3 = dot(AB, BP)  d4 = dot(AC, BP)  d5 = dot(AB, CP)  d6 = dot(AC, CP)
    vc = d1 d4 - d3 d2      vb = d5 d2 - d1 d6      va = d3 d6 - d5 d4
    e = d4 - d3             g = d5 - d6

and the first region of this list whose test holds gives the barycentrics ``(v, w)`` (a comparison with a NaN is false)::

    0 vertex A    d1 <= 0 and d2 <= 0             v = 0               w = 0
    1 vertex B    d3 >= 0 and d4 <= d3            v = 1               w = 0
    2 edge AB     vc <= 0 and d1 >= 0 and d3 <= 0 v = d1 / (d1 - d3)  w = 0
    3 vertex C    d6 >= 0 and d5 <= d6            v = 0               w = 1
    4 edge AC     vb <= 0 and d2 >= 0 and d6 <= 0 v = 0               w = d2 / (d2 - d6)
    5 edge BC     va <= 0 and e >= 0 and g >= 0   w = e / (e + g)     v = 1 - w
    6 interior    otherwise                       s = (va + vb) + vc  v = vb / s   w = vc / s

The closest point is ``X = (A + AB v) + AC w`` per component and ``d2 = ((Px - Xx)^2 + (Py - Xy)^2) + (Pz - Xz)^2``.

Result per query: the minimum over the valid triangles of ``fl32(d2)`` (the float64 value rounded once to float32; an overflow to
``+inf`` is an ordinary value), the lowest triangle index winning a tie; a pair whose ``d2`` is NaN is skipped; a query with no pair
left gets ``(+inf, -1)`` and a NaN point; ``point`` is the winning triangle's ``X`` rounded once to float32.  ``d2`` is a sum of
squares, never negative and never ``-0``: its float32 bit pattern orders like its value, with every NaN above ``+inf``.
"""
from __future__ import annotations

import numpy as np

import metrics_oracle as MO

F32 = np.float32
REGIONS = ("A", "B", "AB", "C", "AC", "BC", "interior")
NAN_KEY = np.uint32(0xFFFFFFFF)
INF_BITS = np.uint32(0x7F800000)


def valid_triangles(v, faces) -> np.ndarray:
    """bool [T]."""
    _, w, ok = MO.face_normals(v, faces)
    return ok & (w > 0)


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def closest_point(P, A, B, C):
    """``(d2 float64 [...], X float64 [..., 3], region int8 [...])`` for float64 arrays of one shape ``[..., 3]`` (the promoted float32
    inputs): the statement of the module docstring, with no validity test."""
    P, A, B, C = (np.asarray(x, dtype=np.float64) for x in (P, A, B, C))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        AB, AC, AP, BP, CP = B - A, C - A, P - A, P - B, P - C
        d1, d2, d3, d4, d5, d6 = _dot(AB, AP), _dot(AC, AP), _dot(AB, BP), _dot(AC, BP), _dot(AB, CP), _dot(AC, CP)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e, g = d4 - d3, d5 - d6
        tests = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e >= 0) & (g >= 0)]
        region = np.full(d1.shape, 6, dtype=np.int8)
        for k in range(5, -1, -1):                                          # the first test that holds wins
            region = np.where(tests[k], np.int8(k), region)
        zero, one = np.zeros_like(d1), np.ones_like(d1)
        w_bc = e / (e + g)
        s = (va + vb) + vc
        v = np.select([region == k for k in range(6)], [zero, one, d1 / (d1 - d3), zero, zero, one - w_bc], vb / s)
        w = np.select([region == k for k in range(6)], [zero, zero, zero, one, d2 / (d2 - d6), w_bc], vc / s)
        X = (A + AB * v[..., None]) + AC * w[..., None]
        D = P - X
        dist2 = (D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1]) + D[..., 2] * D[..., 2]
    return dist2, X, region


def nearest_on_mesh(query, v, faces, rows: int = 256):
    """``(d2 [N] float32, tri [N] int32, point [N, 3] float32)``; ``rows`` queries at a time against all valid triangles."""
    q = np.asarray(query, dtype=F32).reshape(-1, 3)
    v = np.asarray(v, dtype=F32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    N = q.shape[0]
    d2_out = np.full(N, np.inf, dtype=F32)
    tri_out = np.full(N, -1, dtype=np.int32)
    point_out = np.full((N, 3), np.nan, dtype=F32)
    ids = np.flatnonzero(valid_triangles(v, f))
    if ids.size == 0 or N == 0:
        return d2_out, tri_out, point_out
    corners = v.astype(np.float64)[f[ids]]                                   # [Tv, 3 corners, 3]
    A, B, C = corners[None, :, 0], corners[None, :, 1], corners[None, :, 2]
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(0, N, rows):
            P = q[s:s + rows].astype(np.float64)[:, None, :]
            shape = (P.shape[0], ids.size, 3)
            d2, X, _ = closest_point(np.broadcast_to(P, shape), np.broadcast_to(A, shape), np.broadcast_to(B, shape), np.broadcast_to(C, shape))
            d2 = d2.astype(F32)
            key = np.where(np.isnan(d2), NAN_KEY, d2.view(np.uint32))
            arg = key.argmin(axis=1)                                        # the first, i.e. lowest, valid triangle of the minimum
            rng = np.arange(P.shape[0])
            best = key[rng, arg]
            some = best <= INF_BITS
            d2_out[s:s + rows] = np.where(some, best.view(F32), F32(np.inf))
            tri_out[s:s + rows] = np.where(some, ids[arg], -1)
            point_out[s:s + rows] = np.where(some[:, None], X[rng, arg].astype(F32), F32(np.nan))
    return d2_out, tri_out, point_out
