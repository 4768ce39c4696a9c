"""The surface metrics in numpy and Python integers -- TEST INFRASTRUCTURE, the statement tssplat_amd/metrics.py is held to.

Sampler (``sample_surface``).  float32 vertices are promoted to float64; per triangle ``e1 = b - a``, ``e2 = c - a``, the cross
product component-wise as two rounded products and a difference, ``w = sqrt((nx nx + ny ny) + nz nz)``.  A triangle with an index
outside the vertices, a coordinate that is not finite or ``w == 0`` has the integer weight ``q = 0``; every other one
``q = floor((w / w_max) 2^32)`` with ``w_max`` the largest ``w`` (a maximum: order-independent).  ``C`` is the inclusive prefix sum
of ``q`` (Python integers here; associative, so any scan order gives these bits) and ``Q = C[T - 1]``; ``Q == 0`` is an error.
Sample ``i`` draws ``u = mix64(seed, 3 i)`` and takes the first triangle ``t`` with ``C[t] > (u Q) >> 64``: independent, uniform
in area, never a triangle of weight 0.  Its barycentrics are the 24-bit integers ``ia = mix64(seed, 3 i + 1) >> 40`` and
``ib = mix64(seed, 3 i + 2) >> 40``; if ``ia + ib > 2^24`` -- ``a + b > 1`` decided exactly, not after a float32 sum that would
round ``1 + 2^-24`` to 1 -- both are replaced by ``2^24`` minus themselves, and ``a = ia 2^-24``, ``b = ib 2^-24`` are exact in
float32.  The point is ``(A + a (B - A)) + b (C - A)`` in float32, every operation rounded on its own; the normal is the float64
``(nx, ny, nz) / w`` cast to float32.  ``draw`` is everything after the prefix sum, for prefix sums written by hand.

``mix64(seed, c)``: splitmix64's finaliser over ``seed + (c + 1) 0x9E3779B97F4A7C15`` modulo 2^64.

Nearest points (``nearest``).  ``d2 = ((qx - rx)^2 + (qy - ry)^2) + (qz - rz)^2`` in float32 in exactly that order; the minimum
over all ref points; the lower index wins a tie; a pair whose ``d2`` is NaN is skipped; ``+inf`` is an ordinary value; a query
with no pair left returns ``(+inf, -1)``.  ``d2`` is a sum of squares and so never negative and never ``-0``: its bit pattern,
read as an unsigned integer, orders like its value, ``+inf`` included, with every NaN above.

Metrics (``compare``): float64 on the float32 ``d = sqrt(d2)`` (one correctly rounded float32 square root per query).
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

F32 = np.float32
MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def mix64(seed: int, counter: int) -> int:
    z = (seed + (counter + 1) * GOLDEN) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def mix64_array(seed: int, counters: np.ndarray) -> np.ndarray:
    """``mix64`` on a uint64 array of counters (wrapping arithmetic is what uint64 arrays do)."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed & MASK) + (counters.astype(np.uint64) + np.uint64(1)) * np.uint64(GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def face_normals(v, faces):
    """(n [T, 3] float64, w [T] float64, valid [T] bool): the unnormalised normals, their lengths, and which triangles have all
    indices in range and all coordinates finite.  Rows of triangles that are not valid hold zeros."""
    v = np.asarray(v, dtype=F32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    valid = ((f >= 0) & (f < v.shape[0])).all(axis=1)
    g = np.where(valid[:, None], f, 0)
    if v.shape[0] == 0:
        return np.zeros((f.shape[0], 3)), np.zeros(f.shape[0]), np.zeros(f.shape[0], bool)
    p = v.astype(np.float64)[g]                                             # [T, 3 corners, 3]
    valid &= np.isfinite(p).all(axis=(1, 2))
    p = np.where(valid[:, None, None], p, 0.0)
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    w = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
    return n, w, valid


def integer_weights(v, faces) -> np.ndarray:
    """uint64 [T]: ``q``."""
    _, w, valid = face_normals(v, faces)
    w = np.where(valid & np.isfinite(w) & (w > 0), w, 0.0)
    top = w.max() if w.size else 0.0
    if not top > 0:
        return np.zeros(w.shape[0], dtype=np.uint64)
    return np.floor((w / top) * 2.0 ** 32).astype(np.uint64)


def sample_surface(v, faces, n: int, seed: int) -> SimpleNamespace:
    """``points [n, 3] float32, normals [n, 3] float32, tri [n] int32`` and, for the tests, the barycentrics ``a``, ``b``."""
    v = np.asarray(v, dtype=F32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    q = integer_weights(v, f)
    C = np.cumsum([int(x) for x in q], dtype=object) if q.size else np.zeros(0, dtype=object)      # Python integers
    if (int(C[-1]) if q.size else 0) == 0:
        raise RuntimeError("metrics_oracle.sample_surface: faces holds no triangle of positive area")
    s = draw(v, f, C, n, seed)
    s.q = q
    return s


def draw(v, faces, C, n: int, seed: int) -> SimpleNamespace:
    """The part of ``sample_surface`` after the prefix sum: ``n`` samples under the inclusive prefix sums ``C`` (integers, ``[T]``,
    non-decreasing from non-negative weights, ``0 < C[T - 1] < 2^63``), whatever weights they were summed from.  ``p`` is returned too."""
    v = np.asarray(v, dtype=F32).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    C = np.array([int(x) for x in C], dtype=object)
    Q = int(C[-1])
    assert C.shape[0] == f.shape[0] and 0 < Q < 1 << 63
    i = np.arange(n, dtype=np.uint64)
    u = mix64_array(seed, np.uint64(3) * i)
    p = np.array([(int(x) * Q) >> 64 for x in u], dtype=np.uint64)                                # (u Q) >> 64 with Python integers
    tri = np.searchsorted(C.astype(np.uint64), p, side="right").astype(np.int64)                   # the first t with C[t] > p
    ia = (mix64_array(seed, np.uint64(3) * i + np.uint64(1)) >> np.uint64(40)).astype(np.int64)
    ib = (mix64_array(seed, np.uint64(3) * i + np.uint64(2)) >> np.uint64(40)).astype(np.int64)
    flip = ia + ib > 1 << 24
    ia, ib = np.where(flip, (1 << 24) - ia, ia), np.where(flip, (1 << 24) - ib, ib)
    a, b = (ia.astype(F32) * F32(2.0 ** -24)), (ib.astype(F32) * F32(2.0 ** -24))
    A, B, Cc = v[f[tri, 0]], v[f[tri, 1]], v[f[tri, 2]]
    with np.errstate(over="ignore", invalid="ignore"):
        points = ((A + a[:, None] * (B - A)) + b[:, None] * (Cc - A)).astype(F32)
        nrm, w, _ = face_normals(v, f)
        normals = (nrm[tri] / w[tri][:, None]).astype(F32)
    return SimpleNamespace(points=points, normals=normals, tri=tri.astype(np.int32), a=a, b=b, p=p, Q=Q)


NAN_KEY = np.uint32(0xFFFFFFFF)
INF_BITS = np.uint32(0x7F800000)


def nearest(query, ref, rows: int = 1024):
    """``(d2 [N] float32, idx [N] int32)``.  ``rows`` queries at a time against all ref points."""
    q = np.asarray(query, dtype=F32).reshape(-1, 3)
    r = np.asarray(ref, dtype=F32).reshape(-1, 3)
    if r.shape[0] == 0:
        raise RuntimeError("metrics_oracle.nearest: ref holds no point")
    d2_out = np.empty(q.shape[0], dtype=F32)
    idx_out = np.empty(q.shape[0], dtype=np.int32)
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(0, q.shape[0], rows):
            c = q[s:s + rows]
            dx, dy, dz = (c[:, None, k] - r[None, :, k] for k in range(3))
            d2 = ((dx * dx + dy * dy) + dz * dz).astype(F32)
            key = np.where(np.isnan(d2), NAN_KEY, d2.view(np.uint32))
            arg = key.argmin(axis=1)                                        # the first, i.e. lowest, index of the minimum
            best = key[np.arange(c.shape[0]), arg]
            none = best > INF_BITS
            d2_out[s:s + rows] = np.where(none, F32(np.inf), best.view(F32))
            idx_out[s:s + rows] = np.where(none, -1, arg)
    return d2_out, idx_out


def nearest_f64(query, ref, rows: int = 1024):
    """Float64 brute force on finite points: ``(d2_min, idx, d2_second)`` -- the minimum, where, and the smallest value at another index."""
    q = np.asarray(query, dtype=np.float64).reshape(-1, 3)
    r = np.asarray(ref, dtype=np.float64).reshape(-1, 3)
    lo, arg, second = np.empty(q.shape[0]), np.empty(q.shape[0], np.int64), np.empty(q.shape[0])
    for s in range(0, q.shape[0], rows):
        d2 = ((q[s:s + rows, None, :] - r[None, :, :]) ** 2).sum(axis=2)
        a = d2.argmin(axis=1)
        rng = np.arange(d2.shape[0])
        lo[s:s + rows], arg[s:s + rows] = d2[rng, a], a
        d2[rng, a] = np.inf
        second[s:s + rows] = d2.min(axis=1)
    return lo, arg, second


def _one_side(d2, idx, n_self, n_other, thresholds):
    keep = idx >= 0
    d2k = d2[keep]
    with np.errstate(invalid="ignore"):
        d = np.sqrt(d2k).astype(np.float64)                                 # float32 roots, float64 from here on
    count = int(keep.sum())
    side = SimpleNamespace(dropped=int((~keep).sum()), count=count,
                           mean=float(d.sum() / count) if count else float("nan"), max=float(d.max()) if count else float("nan"),
                           mean_sq=float(d2k.astype(np.float64).sum() / count) if count else float("nan"))
    side.counts = [int((d2k <= F32(t) * F32(t)).sum()) for t in thresholds]
    dot = np.abs((n_self[keep, 0].astype(np.float64) * n_other[idx[keep], 0] + n_self[keep, 1].astype(np.float64) * n_other[idx[keep], 1])
                 + n_self[keep, 2].astype(np.float64) * n_other[idx[keep], 2])
    side.normal = float(dot.sum() / count) if count else float("nan")
    return side


def compare(a, b, thresholds=(0.01, 0.02)) -> dict:
    """``a``, ``b``: objects with ``points`` and ``normals``; ``a`` is the surface under test, ``b`` the reference."""
    pa, pb = np.asarray(a.points, dtype=F32), np.asarray(b.points, dtype=F32)
    na, nb = np.asarray(a.normals, dtype=F32), np.asarray(b.normals, dtype=F32)
    d2_ab, idx_ab = nearest(pa, pb)
    d2_ba, idx_ba = nearest(pb, pa)
    ab = _one_side(d2_ab, idx_ab, na, nb.astype(np.float64), thresholds)
    ba = _one_side(d2_ba, idx_ba, nb, na.astype(np.float64), thresholds)
    N, M = pa.shape[0], pb.shape[0]
    rec = {"n_a": N, "n_b": M, "chamfer_l1": 0.5 * (ab.mean + ba.mean), "chamfer_l2": ab.mean_sq + ba.mean_sq, "accuracy": ab.mean, "completeness": ba.mean,
           "accuracy_max": ab.max, "completeness_max": ba.max, "normal_consistency": 0.5 * (ab.normal + ba.normal),
           "dropped_ab": ab.dropped, "dropped_ba": ba.dropped, "thresholds": []}
    for k, t in enumerate(thresholds):
        P, R = ab.counts[k] / N, ba.counts[k] / M
        rec["thresholds"].append({"tau": float(t), "precision": P, "recall": R, "fscore": 2 * P * R / (P + R) if P + R > 0 else 0.0,
                                  "precision_count": ab.counts[k], "recall_count": ba.counts[k]})
    return rec
