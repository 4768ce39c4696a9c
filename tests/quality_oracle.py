"""The definition of tssplat_amd.quality in numpy and Python integers: the lattice snap and the per-triangle record, the crossing
pairs by strict segment / triangle sign tests, the topology counts with union-find over vertices and over corners, and the shape
figures.  The device kernels (csrc/quality_kernels.hip) equal it byte for byte on every integer and on the float64 record.

Everything that decides a crossing is an integer: vertices are snapped to a 2^20 lattice over the cube [lo, hi]^3 first, and the
mesh tested is the snapped mesh (each coordinate moves by at most 2^-21 of the cube's edge).  Strict signs: contacts through a
vertex, along an edge, coplanar overlaps and crossings whose piercings all pass exactly through edges of the other triangle are
NOT counted.
"""
from __future__ import annotations

import numpy as np

LATTICE = 1 << 20
VALID, DEGENERATE, INVALID = 0, 1, 2


# ---- 1. lattice and per-triangle record ----
def snap(v, lo, hi):
    """(X int64 [Nv, 3], ok bool [Nv]): X = floor((double(x) - lo) g + 0.5) with g = (2^20 - 1) / (hi - lo), product and sum rounded
    separately; ok iff the three coordinates are finite and every X lies in 0 .. 2^20 - 1."""
    x = np.asarray(v, np.float32).astype(np.float64).reshape(-1, 3)
    g = np.float64(LATTICE - 1) / (np.float64(hi) - np.float64(lo))
    with np.errstate(invalid="ignore", over="ignore"):
        X = np.floor((x - np.float64(lo)) * g + np.float64(0.5))
        ok = np.isfinite(x).all(1) & (X >= 0).all(1) & (X <= LATTICE - 1).all(1)
    return np.where(ok[:, None], X, 0).astype(np.int64), ok


def cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def prepare(v, faces, lo, hi):
    """(corners int64 [T, 3, 3], state uint8 [T], shape float64 [T, 4]).  state: 0 valid, 1 degenerate (valid, integer cross product
    zero), 2 invalid.  shape, in float64 on the float32 corners, every operation rounded on its own, dot[d] = [dx dx + dy dy] + dz dz:
    dot[b - a], dot[c - b], dot[a - c], dot[(b - a) x (c - a)]; NaN for an invalid triangle.  corners are zero where invalid."""
    v = np.asarray(v, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    T, Nv = faces.shape[0], v.shape[0]
    X, ok = snap(v, lo, hi)
    in_range = ((faces >= 0) & (faces < Nv)).all(1)
    safe = np.where(in_range[:, None], faces, 0)
    valid = in_range & (ok[safe].all(1) if Nv else np.zeros(T, bool))
    corners = np.where(valid[:, None, None], X[safe] if Nv else np.zeros((T, 3, 3), np.int64), 0)
    n = cross(corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0])
    state = np.where(valid, np.where((n == 0).all(1), DEGENERATE, VALID), INVALID).astype(np.uint8)
    p = v.astype(np.float64)[safe] if Nv else np.zeros((T, 3, 3))
    a, b, c = p[:, 0], p[:, 1], p[:, 2]
    dot = lambda d: (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        shape = np.stack([dot(b - a), dot(c - b), dot(a - c), dot(cross(b - a, c - a))], 1)
    shape[~valid] = np.nan
    return corners, state, shape


# ---- 2. crossing pairs ----
def orient(a, b, c, d):
    """det(b - a, c - a, d - a) in int64, expanded along the first row from 2 x 2 minors.  Differences < 2^20, minors < 2^41, terms
    < 2^61, the sum < 3 2^61 < 2^63."""
    a, b, c, d = (np.asarray(x, np.int64) for x in (a, b, c, d))
    u, v, w = b - a, c - a, d - a
    return (u[..., 0] * (v[..., 1] * w[..., 2] - v[..., 2] * w[..., 1]) - u[..., 1] * (v[..., 0] * w[..., 2] - v[..., 2] * w[..., 0])
            + u[..., 2] * (v[..., 0] * w[..., 1] - v[..., 1] * w[..., 0]))


def orient_exact(a, b, c, d):
    """The same determinant in Python integers."""
    u, v, w = ([int(y) - int(x) for x, y in zip(a, p)] for p in (b, c, d))
    return u[0] * (v[1] * w[2] - v[2] * w[1]) - u[1] * (v[0] * w[2] - v[2] * w[0]) + u[2] * (v[0] * w[1] - v[1] * w[0])


def pierces(p, q, a, b, c):
    sp, sq = orient(a, b, c, p), orient(a, b, c, q)
    o1, o2, o3 = orient(p, q, a, b), orient(p, q, b, c), orient(p, q, c, a)
    straddles = ((sp > 0) & (sq < 0)) | ((sp < 0) & (sq > 0))
    return straddles & (((o1 > 0) & (o2 > 0) & (o3 > 0)) | ((o1 < 0) & (o2 < 0) & (o3 < 0)))


def crosses(A, B):
    """A, B int64 [..., 3, 3]: an edge of one pierces the other (six segment / triangle tests)."""
    hit = np.zeros(A.shape[:-2], bool)
    for k in range(3):
        hit |= pierces(A[..., k, :], A[..., (k + 1) % 3, :], B[..., 0, :], B[..., 1, :], B[..., 2, :])
        hit |= pierces(B[..., k, :], B[..., (k + 1) % 3, :], A[..., 0, :], A[..., 1, :], A[..., 2, :])
    return hit


def self_intersections(v, faces, lo, hi, rows=256):
    """dict: crossings int32 [T], pairs int64 sorted keys i << 32 | j (i < j), crossing_pairs, crossing_faces, invalid_faces,
    degenerate_faces, box_pairs (valid, non-degenerate pairs i < j whose closed lattice boxes overlap), state."""
    corners, state, _ = prepare(v, faces, lo, hi)
    T = corners.shape[0]
    good = state == VALID
    bmin, bmax = corners.min(1), corners.max(1)
    crossings = np.zeros(T, np.int32)
    keys = []
    box_pairs = 0
    idx = np.arange(T)
    for r0 in range(0, T, rows):
        r1 = min(T, r0 + rows)
        ov = good[r0:r1, None] & good[None, :] & (idx[None, :] > idx[r0:r1, None])
        for k in range(3):
            ov &= (bmin[r0:r1, None, k] <= bmax[None, :, k]) & (bmin[None, :, k] <= bmax[r0:r1, None, k])
        i, j = np.nonzero(ov)
        i += r0
        box_pairs += int(i.size)
        if i.size:
            hit = crosses(corners[i], corners[j])
            i, j = i[hit], j[hit]
            np.add.at(crossings, i, 1)
            np.add.at(crossings, j, 1)
            keys.append((i.astype(np.int64) << 32) | j.astype(np.int64))
    pairs = np.sort(np.concatenate(keys)) if keys else np.zeros(0, np.int64)
    return dict(crossings=crossings, pairs=pairs, crossing_pairs=int(pairs.size), crossing_faces=int((crossings > 0).sum()),
                invalid_faces=int((state == INVALID).sum()), degenerate_faces=int((state == DEGENERATE).sum()), box_pairs=box_pairs, state=state)


# ---- 3. topology ----
def _find(L, x):
    while L[x] != x:
        L[x] = L[L[x]]
        x = L[x]
    return x


def _union(L, a, b):
    a, b = _find(L, a), _find(L, b)
    if a != b:
        L[max(a, b)] = min(a, b)


def topology(faces, n_vertices, valid=None):
    """All counts over the valid triangles (``valid`` bool [T]; None: those with indices in range).  Half-edge 3 t + k runs from
    faces[t, k] to faces[t, (k + 1) % 3] and corner 3 t + k sits at faces[t, k].  Two half-edges with the same undirected key join, at
    each end x of the first, its corner there with the second's corner at x (the second's first corner if that sits at x, else its
    second)."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    T, Nv = faces.shape[0], int(n_vertices)
    if valid is None:
        valid = ((faces >= 0) & (faces < Nv)).all(1)
    valid = np.asarray(valid, bool)
    tv = np.nonzero(valid)[0]
    f = faces[tv]
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
    half = (3 * tv[:, None] + np.arange(3)[None, :]).reshape(-1)
    und = (np.minimum(a, b) << 32) | np.maximum(a, b)
    _, counts = np.unique(und, return_counts=True)
    directed = np.unique((a << 32) | b)
    edges, boundary, nonmanifold = int(counts.size), int((counts == 1).sum()), int((counts > 2).sum())
    repeated = int(a.size - directed.size)
    referenced = np.zeros(Nv, bool)
    referenced[f.reshape(-1)] = True
    L = list(range(Nv))
    for x, y in zip(a.tolist(), b.tolist()):
        _union(L, x, y)
    component = np.array([_find(L, x) if referenced[x] else -1 for x in range(Nv)], np.int32).reshape(Nv)
    C = list(range(3 * T))
    order = np.argsort(und, kind="stable")
    flat = faces.reshape(-1)
    for p in range(1, order.size):
        if und[order[p]] != und[order[p - 1]]:
            continue
        h1, h2 = int(half[order[p - 1]]), int(half[order[p]])
        t1, k1, t2, k2 = h1 // 3, h1 % 3, h2 // 3, h2 % 3
        for e in range(2):
            c1 = 3 * t1 + (k1 + e) % 3
            c2 = 3 * t2 + k2 if flat[3 * t2 + k2] == flat[c1] else 3 * t2 + (k2 + 1) % 3
            _union(C, c1, c2)
    fans = np.zeros(Nv, np.int32)
    for c in half.tolist():
        if _find(C, c) == c:
            fans[flat[c]] += 1
    nmv = int((fans > 1).sum())
    return dict(edges=edges, boundary_edges=boundary, nonmanifold_edges=nonmanifold, repeated_directed_edges=repeated, oriented=repeated == 0,
                components=int((component == np.arange(Nv)).sum()), component=component, fans=fans, nonmanifold_vertices=nmv,
                manifold=nonmanifold == 0 and nmv == 0, euler=int(referenced.sum()) - edges + int(tv.size), valid_faces=int(tv.size),
                referenced_vertices=int(referenced.sum()), closed=bool((counts == 2).all() and repeated == 0))


# ---- 4. shape figures ----
def shape_figures(shape):
    """From the float64 record of the valid triangles: alr = 12 sqrt(3) A / P^2 and the minimum angle in degrees, per triangle."""
    s = shape[np.isfinite(shape).all(1)]
    l = np.sqrt(s[:, :3])
    area, per = 0.5 * np.sqrt(s[:, 3]), l.sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        alr = np.where(per > 0, 12.0 * np.sqrt(3.0) * area / (per * per), 0.0)
        # the smallest angle is opposite the shortest edge: sin = 2 A / (product of the other two edges), cos from the law of cosines
        k = np.argmin(s[:, :3], 1)
        r = np.arange(s.shape[0])
        e0, e1, e2 = s[r, k], s[r, (k + 1) % 3], s[r, (k + 2) % 3]
        ang = np.degrees(np.arctan2(np.sqrt(s[:, 3]), 0.5 * (e1 + e2 - e0)))
    return alr, np.where(np.isfinite(ang), ang, 0.0)
