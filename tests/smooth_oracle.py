"""Oracle of the surface smoother (tssplat_amd/smooth.py; tsamd_smooth_*): numpy, float64, every operation rounded on its own.  This
file is the definition; the device results equal it byte for byte.

Valid face: three indices in 0 .. Nv - 1, pairwise distinct.  Nothing else contributes to anything.
Neighbours N(i): the distinct vertices sharing an edge of a valid face with i, ascending.  Edge-irregular: i lies on an undirected
edge that is in some number of valid faces other than two (a face listed twice counts twice).
State: float64 from double(v), rounded to float32 once at the end.  A vertex moves iff it is finite, has a neighbour, all its
neighbours are finite in the INPUT, it is not pinned, and (boundary = "free" or it is not edge-irregular); every other vertex keeps
its input bits and is counted under the first reason that holds: other, pinned, irregular.
Umbrella: L_i = (sum of p_j over N(i) ascending, per component, sequential from 0.0) / double(deg_i) - p_i.
A half-step with coefficient c (one whose c == 0.0 is skipped, in either mode) reads only the state before it:
  taubin       p <- p + c L;  one iteration is the half-step lam, then the half-step mu
  tangential   d = c L;  n = sum over the valid faces t containing i, ascending t, sequential from 0.0, of N_t = cross(p_b - p_a, p_c - p_a)
               (a, b, c the face's corners in its own order; a component is a difference of two rounded products);
               nn = (nx nx + ny ny) + nz nz;  if nn > 0: s = ((dx nx + dy ny) + dz nz) / nn and p <- p + (d - n s), else p stays;
               one iteration is the half-step lam
max_move = r: after every half-step each coordinate q becomes lo if q < lo, else hi if q > hi, else q, with lo = p0 - r and hi = p0 + r
rounded once from the float64 input p0 (a NaN passes through: nothing is special-cased beyond IEEE).
"""
import numpy as np

F64 = np.float64
MAX_ITERATIONS = 4096


def adjacency(faces, n_vertices):
    """dict(offsets int32 [Nv + 1], neighbours int32, face_offsets int32 [Nv + 1], faces_of int32, irregular uint8 [Nv], valid uint8 [Nt])."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    Nv = int(n_vertices)
    a, b, c = f[:, 0], f[:, 1], f[:, 2]
    valid = ((f >= 0) & (f < Nv)).all(1) & (a != b) & (b != c) & (a != c)
    tv = np.nonzero(valid)[0]
    g = f[tv]
    src = np.concatenate([g[:, 0], g[:, 1], g[:, 1], g[:, 2], g[:, 2], g[:, 0]])
    dst = np.concatenate([g[:, 1], g[:, 0], g[:, 2], g[:, 1], g[:, 0], g[:, 2]])
    keys, count = np.unique((src << 32) | dst, return_counts=True)          # ascending: by source, then by neighbour
    rows = keys >> 32
    irregular = np.zeros(Nv, np.uint8)
    irregular[rows[count != 2]] = 1
    offsets = np.searchsorted(rows, np.arange(Nv + 1)).astype(np.int32)
    fkeys = np.sort(((g.reshape(-1)) << 32) | np.repeat(tv, 3))             # unique: a valid face names a vertex once
    face_offsets = np.searchsorted(fkeys >> 32, np.arange(Nv + 1)).astype(np.int32)
    return dict(offsets=offsets, neighbours=(keys & 0xFFFFFFFF).astype(np.int32), face_offsets=face_offsets,
                faces_of=(fkeys & 0xFFFFFFFF).astype(np.int32), irregular=irregular, valid=valid.astype(np.uint8))


HELD_NAMES = ("moved", "held_other", "held_pinned", "held_irregular")


def classify(v, adj, boundary="fixed", pinned=None):
    """uint8 [Nv]: 0 moves, 1 held for another reason (not finite, a neighbour not finite, no neighbour), 2 pinned, 3 edge-irregular."""
    v = np.asarray(v, np.float32).reshape(-1, 3)
    Nv = v.shape[0]
    finite = np.isfinite(v).all(1)
    off, nb = adj["offsets"].astype(np.int64), adj["neighbours"].astype(np.int64)
    deg = off[1:] - off[:-1]
    bad_nb = np.zeros(Nv, bool)
    np.logical_or.at(bad_nb, np.repeat(np.arange(Nv), deg), ~finite[nb])
    cls = np.zeros(Nv, np.uint8)
    if boundary == "fixed":
        cls[adj["irregular"] != 0] = 3
    if pinned is not None:
        cls[np.asarray(pinned, bool)] = 2
    cls[~finite | bad_nb | (deg == 0)] = 1
    return cls


def _clamp(q, lo, hi):
    with np.errstate(invalid="ignore"):
        return np.where(q < lo, lo, np.where(q > hi, hi, q))


def umbrella(p, adj):
    """float64 [Nv, 3]: L_i; NaN rows where deg = 0 (those vertices never move)."""
    off, nb = adj["offsets"].astype(np.int64), adj["neighbours"].astype(np.int64)
    Nv = p.shape[0]
    deg = off[1:] - off[:-1]
    acc = np.zeros((Nv, 3), F64)
    for k in range(int(deg.max()) if Nv else 0):                            # the k-th neighbour of every row that has one: sequential per row
        rows = np.nonzero(deg > k)[0]
        with np.errstate(invalid="ignore", over="ignore"):
            acc[rows] = acc[rows] + p[nb[off[rows] + k]]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return acc / deg.astype(F64)[:, None] - p


def vertex_normals(p, faces, adj):
    """float64 [Nv, 3]: the sum of N_t over a vertex's valid faces in ascending t, sequential from 0.0."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    off, fo = adj["face_offsets"].astype(np.int64), adj["faces_of"].astype(np.int64)
    Nv = p.shape[0]
    cnt = off[1:] - off[:-1]
    N = np.zeros((f.shape[0], 3), F64)
    tv = np.nonzero(adj["valid"] != 0)[0]
    with np.errstate(invalid="ignore", over="ignore"):
        a, b, c = p[f[tv, 0]], p[f[tv, 1]], p[f[tv, 2]]
        u, w = b - a, c - a
        N[tv] = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
        acc = np.zeros((Nv, 3), F64)
        for k in range(int(cnt.max()) if Nv else 0):
            rows = np.nonzero(cnt > k)[0]
            acc[rows] = acc[rows] + N[fo[off[rows] + k]]
    return acc


def half_step(p, faces, adj, move, mode, coef, p0=None, max_move=None):
    """One half-step of the float64 state ``p`` -> a new array; ``move`` bool [Nv]."""
    coef = F64(coef)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        L = umbrella(p, adj)
        if mode == "taubin":
            q = p + coef * L
        else:
            d = coef * L
            n = vertex_normals(p, faces, adj)
            nn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
            s = ((d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]) / nn
            q = np.where((nn > 0)[:, None], p + (d - n * s[:, None]), p)
        if max_move is not None:
            r = F64(max_move)
            q = _clamp(q, p0 - r, p0 + r)
    return np.where(move[:, None], q, p)


def coefficients(mode, lam, mu):
    """The half-steps of one iteration, the exactly-zero ones left out."""
    return [c for c in ((lam, mu) if mode == "taubin" else (lam,)) if F64(c) != 0.0]


def smooth(v, faces, iterations=10, mode="taubin", lam=0.5, mu=-0.53, boundary="fixed", pinned=None, max_move=None, adj=None):
    """dict(v float32 [Nv, 3], state float64 (the unrounded result), cls, moved, held_other, held_pinned, held_irregular)."""
    assert mode in ("taubin", "tangential") and boundary in ("fixed", "free") and 0 <= iterations <= MAX_ITERATIONS
    v = np.ascontiguousarray(v, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    adj = adjacency(faces, v.shape[0]) if adj is None else adj
    cls = classify(v, adj, boundary, pinned)
    move = cls == 0
    p0 = v.astype(F64)
    p = p0.copy()
    for _ in range(iterations):
        for c in coefficients(mode, lam, mu):
            p = half_step(p, faces, adj, move, mode, c, p0, max_move)
    with np.errstate(invalid="ignore", over="ignore"):
        out = np.where(move[:, None], p.astype(np.float32), v)
    out = out.view(np.uint32)
    out[~move] = v.view(np.uint32)[~move]                                   # the input's bits, whatever np.where makes of a NaN's payload
    counts = np.bincount(cls, minlength=4)
    return dict(v=out.view(np.float32), state=p, cls=cls, **{k: int(counts[i]) for i, k in enumerate(HELD_NAMES)})


# ---- figures for the tests that check the oracle against what is known ----
def alr(v, faces):
    """12 sqrt(3) A / P^2 per face, float64."""
    v, f = np.asarray(v, F64), np.asarray(faces, np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    per = np.linalg.norm(b - a, axis=1) + np.linalg.norm(c - b, axis=1) + np.linalg.norm(a - c, axis=1)
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    return 12.0 * np.sqrt(3.0) * area / (per * per)


def volume(v, faces):
    v, f = np.asarray(v, F64), np.asarray(faces, np.int64)
    return float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)
