"""Per-entry error bounds, fp32 emulations and small topologies for the surface glue -- TEST INFRASTRUCTURE.

The float64 statements are those of oracle/surface_oracle.py (pinned to the reference's goldens); everything here is built on
top of it.  ``bounds()`` evaluates them on float64 copies of fp32 inputs and returns, next to every quantity, the largest error
an fp32 implementation (``U = 2^-24``) of the chain in the header comments of csrc/surface_kernels.hip can make in that entry.
The counts hold whether each operation is rounded on its own, the cross products are fused (``fma(a, b, -(c d))``), or the
running sum is fused too (``fma(a, b, fma(-c, d, acc))``): the translation unit is built with ``-ffp-contract=fast``.

Notation: vertex ``v`` has the incidence list ``j = 1 .. k_v`` (faces ascending, a face that names the vertex twice twice),
``M_j = |e1| (x) |e2|`` is entry j's cross product with every term taken positive (componentwise, float64),
``P_j = M_1 + .. + M_j`` and ``S_v = P_k``.

* Raw normal, componentwise: ``B_raw = U (6 S_v + 2 (P_1 + .. + P_{k-1}))``.  Each edge is one rounding (2 per product, ``2 U M_j``).
  Rounded separately a face adds one rounding per product and one for the difference (``2 U M_j``) and the running sum one per
  face after the first, each at most ``U P_j``: ``4 U S_v + U (P_2 + .. + P_k)``.  Fully fused every face costs two roundings of
  a partial sum, each at most ``U P_j``: ``2 U S_v + 2 U (P_1 + .. + P_k)``.  The stated bound covers both with ``U S_v`` to spare
  for the second-order terms (k <= 300).  It never exceeds ``(2 k + 4) U S_v`` and is ``(k + 5) U S_v`` on a fan of equal faces.
* Unit normal, componentwise: ``2 beta + 5 U`` with ``beta = ||B_raw|| / |n|``: ``|a / |a| - b / |b|| <= 2 |a - b| / |b|`` for the raw
  error; |n|^2 is 3 positive products and 2 sums (3 U), the root halves that and adds one, the reciprocal one, the product one.
* ``h = (g - nh (nh . g)) / |n|``, componentwise: ``(3 beta + 20 U) |g| / |n|`` for ``beta <= 1/4`` (``inf`` above: no test may rest on
  such a vertex).  The direction error (at most ``beta (1 + beta)``) moves the projector by as much, ``1 / |n|`` moves by ``beta / (1 -
  beta)``: ``2 beta`` plus at most ``4 beta^2 <= beta``.  Roundings: the common factor ``1 / |n|`` enters the projected term twice (7 U),
  the three products of the unit normal (2 U), the dot product (3 U), product and difference (2 U), the final product by
  ``1 / |n|`` (4.5 U): 18.5 U.
* Positions gradient, componentwise.  Entry j contributes ``+-e x G`` with ``G = h_0 + h_1 + h_2`` (``dG``: the three h bounds plus
  ``2 U sum |h|``) and the absolute mass ``A_j = |e| (x) |G|`` (corner 0: both cross products).  Per entry ``5 U A_j + |e| (x) dG``
  (edge, product, difference, the sum of corner 0, one to spare); the accumulation adds at most ``r_j U Q_j`` with ``Q_j = A_1 + ..
  + A_j`` and ``r_j`` the most roundings of a partial sum a fused entry can make (2, corner 0: 4).
* Underflow: every bound above gains ``8 k_v 2^-126`` where it is not zero, which covers gradual underflow and flush to zero.
* Exactness: where the reference is exactly 0 by construction -- a vertex with no face, a replaced normal's h, the rows of
  ``grad_tet_v`` outside ``surface_vid`` -- the bound is 0 and so is every replaced unit normal's ((0, 0, 1) exactly).  The gather
  and its adjoint on distinct ids move bits.

Worst error / bound of the emulations below on the GPU size matrix of tests/test_surface.py (measured against the float64
oracle, never against a kernel), rounded separately | fused:

    raw normal 0.39 | 0.32    unit normal 0.097 | 0.097    h 0.079 | 0.074    positions gradient 0.027 | 0.023

(The gradient bound is loose because it carries the worst case of the raw normal through ``beta``, which no fan comes near.)

``emulate_*`` restate the header comments in fp32 numpy, every operation rounded on its own or (``fused``) with the multiply-adds
fused as above, faces in ascending order.  ``mutation`` names one deliberate fault (``MUTATIONS``); tests/test_surface.py shows
on the CPU that the correct emulations stay inside every bound and that every mutant leaves one on a named case.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from oracle import surface_oracle as SO

U = 2.0 ** -24
TINY = 2.0 ** -126
THRESHOLD = 1e-20
BAND = 16 * U               # relative half-width around THRESHOLD inside which either decision is a correct fp32 one
F32 = np.float32

MUTATIONS = ("skip_last_entry", "skip_corner2", "norm_threshold", "keep_h", "overwrite_duplicates", "corner0_as_corner1")


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _abscross(a, b):
    a, b = np.abs(a), np.abs(b)
    return np.stack([a[:, 1] * b[:, 2] + a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] + a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0]], axis=1)


def incidence(faces, nv):
    """(off [nv + 1], ent [3 nf]): vertex v's entries ``4 * face + corner`` are ent[off[v] : off[v + 1]], faces ascending."""
    flat = np.asarray(faces, dtype=np.int64).reshape(-1)
    order = np.argsort(flat, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=nv))]).astype(np.int64)
    return off, (4 * (order // 3) + order % 3).astype(np.int64)


def _segsum(x, owner, nv):
    out = np.zeros((nv,) + x.shape[1:])
    np.add.at(out, owner, x)
    return out


def _prefix(x, off, owner):
    """Inclusive running sum of the rows of x within every vertex's list."""
    c = np.concatenate([np.zeros((1,) + x.shape[1:]), np.cumsum(x, axis=0)])
    return c[1:] - c[off[:-1]][owner]


def bounds(v_pos, faces, grad_nrm=None, kept=None):
    """Float64 reference and per-entry bound of raw normal, unit normal and -- with ``grad_nrm`` -- h and the positions gradient.
    ``kept`` (boolean per vertex) overrides the reference's ``|n|^2 > 1e-20`` where a test has to follow a decision made inside
    the band.  ``undecided``: vertices whose decision an fp32 implementation may make either way."""
    v, f = _f64(v_pos), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    nv = v.shape[0]
    off, ent = incidence(f, nv)
    k = np.diff(off)
    owner = np.repeat(np.arange(nv), k)
    ef, ec = ent >> 2, ent & 3
    e1, e2 = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        M = _abscross(e1, e2)[ef]
        S = _segsum(M, owner, nv)
        under = 8 * k[:, None] * TINY
        r = SimpleNamespace(off=off, ent=ent, k=k, S=S)
        r.raw = SO._raw_normals(v, f)
        r.b_raw = U * (4 * S + 2 * _segsum(_prefix(M, off, owner), owner, nv)) + under * (S > 0)
        nn = (r.raw * r.raw).sum(axis=1)
        r.nn = nn
        r.beta = np.where(nn > 0, np.linalg.norm(r.b_raw, axis=1) / np.sqrt(np.where(nn > 0, nn, 1.0)), 0.0)
        ln0, lb = np.sqrt(nn), np.linalg.norm(r.b_raw, axis=1)
        r.undecided = (np.maximum(ln0 - lb, 0) ** 2 <= THRESHOLD * (1 + BAND)) & ((ln0 + lb) ** 2 >= THRESHOLD * (1 - BAND))
        r.kept = nn > THRESHOLD if kept is None else np.asarray(kept, dtype=bool)
        ok = r.kept[:, None]
        ln = np.sqrt(np.where(r.kept, nn, 1.0))[:, None]
        nh = np.where(ok, r.raw / ln, np.array([0.0, 0.0, 1.0]))
        r.nrm = nh
        r.b_nrm = np.where(ok, 2 * r.beta[:, None] + 5 * U, 0.0) * np.ones(3)
        r.cond = np.where(nn > 0, np.linalg.norm(S, axis=1) / np.sqrt(np.where(nn > 0, nn, 1.0)), 0.0)
        if grad_nrm is None:
            return r
        g = _f64(grad_nrm)
        r.h = np.where(ok, (g - nh * (nh * g).sum(axis=1, keepdims=True)) / ln, 0.0)
        bh = (3 * r.beta + 20 * U) * np.linalg.norm(g, axis=1) / ln[:, 0]
        bh = np.where(r.beta <= 0.25, bh, np.inf)
        r.b_h = np.where(ok, bh[:, None], 0.0) * np.ones(3)
        G = r.h[f[:, 0]] + r.h[f[:, 1]] + r.h[f[:, 2]]
        dG = r.b_h[f[:, 0]] + r.b_h[f[:, 1]] + r.b_h[f[:, 2]] + 2 * U * (np.abs(r.h[f[:, 0]]) + np.abs(r.h[f[:, 1]]) + np.abs(r.h[f[:, 2]]))
        d1, d2 = np.cross(e2, G), np.cross(G, e1)
        a1, a2 = _abscross(e2, G), _abscross(G, e1)
        p1, p2 = _abscross(e2, dG), _abscross(dG, e1)
        c = ec[:, None]
        term = np.where(c == 1, d1[ef], np.where(c == 2, d2[ef], -(d1 + d2)[ef]))
        A = np.where(c == 1, a1[ef], np.where(c == 2, a2[ef], (a1 + a2)[ef]))
        prop = np.where(c == 1, p1[ef], np.where(c == 2, p2[ef], (p1 + p2)[ef]))
        prop = np.where(prop > 0, prop, 0.0)                                     # 0 * inf: an exact zero edge propagates nothing
        rounds = np.where(c == 0, 4.0, 2.0)
        r.grad = _segsum(term, owner, nv)
        mass = _segsum(A, owner, nv)
        r.b_grad = (_segsum(5 * U * A + prop * (1 + 8 * U), owner, nv) + U * _segsum(rounds * _prefix(A, off, owner), owner, nv)
                    + under * ((mass > 0) | (_segsum(prop, owner, nv) > 0)))
    return r


def ratio(got, ref, bound):
    """Worst |got - ref| / bound; an entry whose bound is 0 must be +-0 where the reference is (inf otherwise)."""
    err = np.abs(_f64(got) - ref)
    if err.size == 0:
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    q = np.where(np.isnan(q), np.inf, q)
    return float(q.max())


# ---- fp32 emulations ----------------------------------------------------------------------------------------------------------

def _fma(a, b, c):
    """a * b + c, the product unrounded (exact in float64), the sum rounded to fp32."""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F32)


def _cross_into(acc, a, b, fused, sign=1.0):
    """acc + sign * (a x b) on [m, 3] fp32 arrays."""
    out = np.empty_like(acc)
    s = F32(sign)
    for i, (p, q) in enumerate(((1, 2), (2, 0), (0, 1))):
        if fused:
            out[:, i] = _fma(s * a[:, p], b[:, q], _fma(-s * a[:, q], b[:, p], acc[:, i]))
        else:
            out[:, i] = acc[:, i] + s * (a[:, p] * b[:, q] - a[:, q] * b[:, p])
    return out


def _dot(a, b, fused):
    if fused:
        return _fma(a[:, 2], b[:, 2], _fma(a[:, 1], b[:, 1], a[:, 0] * b[:, 0]))
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def _lists(faces, nv, mutation):
    off, ent = incidence(faces, nv)
    k = np.diff(off)
    if mutation == "skip_last_entry":
        k = np.maximum(k - 1, 0)
    return off, ent, k


def emulate_normals(v_pos, faces, fused=False, mutation=None, drop_below=None):
    """(raw, v_nrm) in fp32.  ``drop_below``: skip every entry whose face has |e1 x e2| below that fraction of its fan's sum of
    them (the mutant of the old-tolerance comparison)."""
    v, f = np.asarray(v_pos, dtype=F32), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    nv = v.shape[0]
    off, ent, k = _lists(f, nv, mutation)
    skip = np.zeros(ent.shape[0], dtype=bool)
    if drop_below is not None:
        area = np.linalg.norm(np.cross(_f64(v)[f[:, 1]] - _f64(v)[f[:, 0]], _f64(v)[f[:, 2]] - _f64(v)[f[:, 0]]), axis=1)[ent >> 2]
        owner = np.repeat(np.arange(nv), np.diff(off))
        skip = area < drop_below * _segsum(area, owner, nv)[owner]
    raw = np.zeros((nv, 3), F32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        for j in range(int(k.max()) if nv else 0):
            act = np.nonzero(k > j)[0]
            e = off[act] + j
            act, e = act[~skip[e]], e[~skip[e]]
            t = f[ent[e] >> 2]
            p0 = v[t[:, 0]]
            raw[act] = _cross_into(raw[act], v[t[:, 1]] - p0, v[t[:, 2]] - p0, fused)
        nn = _dot(raw, raw, fused)
        test = np.sqrt(nn) if mutation == "norm_threshold" else nn
        n = np.where((test > F32(THRESHOLD))[:, None], raw, np.array([0, 0, 1], F32))
        inv = F32(1) / np.maximum(np.sqrt(_dot(n, n, fused)), F32(1e-12))
        return raw, n * inv[:, None]


def emulate_normals_backward(v_pos, faces, raw, grad_nrm, fused=False, mutation=None):
    """(h, grad_v_pos) in fp32 from the stored raw normals."""
    v, f = np.asarray(v_pos, dtype=F32), np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    n, g = np.asarray(raw, dtype=F32), np.asarray(grad_nrm, dtype=F32)
    nv = v.shape[0]
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        nn = _dot(n, n, fused)
        test = np.sqrt(nn) if mutation == "norm_threshold" else nn
        inv = F32(1) / np.maximum(np.sqrt(nn), F32(1e-12))
        nh = n * inv[:, None]
        t = _dot(nh, g, fused)
        if fused:
            h = _fma(-nh, t[:, None], g) * inv[:, None]
        else:
            h = (g - nh * t[:, None]) * inv[:, None]
        if mutation != "keep_h":
            h = np.where((test > F32(THRESHOLD))[:, None], h, F32(0)).astype(F32)
        off, ent, k = _lists(f, nv, mutation)
        acc = np.zeros((nv, 3), F32)
        for j in range(int(k.max()) if nv else 0):
            act = np.nonzero(k > j)[0]
            e = ent[off[act] + j]
            t3, corner = f[e >> 2], e & 3
            if mutation == "corner0_as_corner1":
                corner = np.where(corner == 0, 1, corner)
            p0 = v[t3[:, 0]]
            e1, e2 = v[t3[:, 1]] - p0, v[t3[:, 2]] - p0
            G = (h[t3[:, 0]] + h[t3[:, 1]]) + h[t3[:, 2]]
            a = acc[act]
            one = _cross_into(a, e2, G, fused)                                              # corner 1: + e2 x G
            two = _cross_into(a, G, e1, fused)                                              # corner 2: + G x e1
            if mutation == "skip_corner2":
                two = a
            zero = np.zeros_like(a)
            if fused:
                both = _cross_into(_cross_into(a, e2, G, True, -1.0), G, e1, True, -1.0)
            else:
                both = a - (_cross_into(zero, e2, G, False) + _cross_into(zero, G, e1, False))
            c = corner[:, None]
            acc[act] = np.where(c == 1, one, np.where(c == 2, two, both))
        return h, acc


def emulate_positions(tet_v, surface_vid):
    return np.asarray(tet_v, dtype=F32)[np.asarray(surface_vid, dtype=np.int64)]


def emulate_positions_backward(grad_v_pos, surface_vid, n_tet_vertices, mutation=None):
    g, vid = np.asarray(grad_v_pos, dtype=F32), np.asarray(surface_vid, dtype=np.int64)
    out = np.zeros((n_tet_vertices, 3), F32)
    if mutation == "overwrite_duplicates":
        out[vid] = g
    else:
        np.add.at(out, vid, g)
    return out


# ---- topologies ---------------------------------------------------------------------------------------------------------------

def soup(nv, nf, seed=0):
    """nf triangles whose corners are drawn independently from nv vertices: faces that repeat a vertex and vertices with no
    face occur."""
    return np.random.default_rng(10_000 + 7 * nv + nf + seed).integers(0, nv, (nf, 3)).astype(np.int32)


def hub(k):
    """Vertex 0 in k faces around a ring of k vertices; the hub takes corner j % 3 of face j."""
    j = np.arange(k)
    f = np.stack([np.zeros(k, np.int64), 1 + j, 1 + (j + 1) % k], axis=1)
    return np.stack([np.roll(row, s) for row, s in zip(f, j % 3)]).astype(np.int32)


def hub_positions(k, seed=0):
    """The ring winds k / 10 times around the hub, 36 degrees a face: no face is a sliver, all agree in orientation (that they
    overlap in space is nothing to the kernels), so neither a cross product nor the fan of the hub cancels."""
    rng = np.random.default_rng(20_000 + k + seed)
    a = 2 * np.pi * (np.arange(k) + rng.uniform(-0.2, 0.2, k)) / 10
    r = rng.uniform(0.5, 1.5, k)
    ring = np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-0.1, 0.1, k)], axis=1)
    return np.concatenate([[[0.01, -0.02, 0.3]], ring]).astype(F32)


def isolated_triangles(T):
    return np.arange(3 * T, dtype=np.int32).reshape(T, 3)


def conditioned_positions(faces, nv, seed=0, limit=8.0):
    """fp32 positions uniform in [-1, 1]^3 in which no fan cancels worse than ``||S_v|| / |n| <= limit``.  The vertex of a fan
    that does is drawn again until its own fan passes and no fan that passed before fails -- alone for 50 attempts, then with
    1, 2, .. other vertices of its fan (a long fan hardly depends on its own vertex).  Every other vertex keeps its first draw.
    Returns (positions, number of vertices drawn again).  A soup with 2 nv faces has 3 % to 9 % such fans, depending on the seed."""
    rng = np.random.default_rng(seed)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    v = rng.uniform(-1, 1, (nv, 3)).astype(F32)
    bad = set(np.nonzero(bounds(v, f).cond > limit)[0].tolist())
    redrawn = set(bad)
    for vtx in sorted(bad):
        if vtx not in bad:
            continue
        others = np.setdiff1d(f[np.any(f == vtx, axis=1)].reshape(-1), [vtx])
        for attempt in range(1000):
            move = [vtx] + rng.choice(others, min(attempt // 50, others.size), replace=False).tolist()
            w = v.copy()
            w[move] = rng.uniform(-1, 1, (len(move), 3)).astype(F32)
            now = set(np.nonzero(bounds(w, f).cond > limit)[0].tolist())
            if now <= bad - {vtx}:
                v, bad = w, now
                redrawn.update(move)
                break
        else:
            raise AssertionError("conditioned_positions: no position found for a fan")
    assert not bad
    return v, len(redrawn)


def lattice_sheet(nx, ny, heights=None):
    """(positions, faces) of an (nx + 1) x (ny + 1) integer grid whose cells are split along alternating diagonals, so that
    every vertex lies in 1, 2, 4 or 8 triangles.  Flat (``heights`` None) every raw normal is (0, 0, 2^m); with integer heights
    in [0, 3] every product and sum of the raw normals stays a small integer: exact in fp32, fused or not."""
    ix, iy = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="ij")
    z = np.zeros_like(ix) if heights is None else np.asarray(heights).reshape(nx + 1, ny + 1)
    v = np.stack([ix, iy, z], axis=-1).reshape(-1, 3).astype(F32)
    idx = lambda i, j: i * (ny + 1) + j
    faces = []
    for i in range(nx):
        for j in range(ny):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            faces += [[a, b, c], [c, d, a]] if (i + j) % 2 == 0 else [[b, c, d], [d, a, b]]
    return v, np.asarray(faces, dtype=np.int32)


def threshold_triangles(targets):
    """Positions of isolated triangles whose float64 |n|^2 is ``targets`` (to about 2^-35 relative) with the normal along
    (small, 0, -1): p0 = 0, e1 = (0, a, 0), e2 = (b, 0, c), n = (a c, 0, -a b), a = 2^-17, b just below sqrt(target) / a and c
    making up the rest.  Every product by a is exact."""
    t = _f64(targets)
    a = 2.0 ** -17
    b = (np.sqrt(t) / a * (1 - 2.0 ** -12)).astype(F32).astype(np.float64)
    c = np.sqrt(t / a ** 2 - b ** 2).astype(F32).astype(np.float64)
    v = np.zeros((t.size, 3, 3))
    v[:, 1, 1] = a
    v[:, 2, 0], v[:, 2, 2] = b, c
    return v.reshape(-1, 3).astype(F32)
