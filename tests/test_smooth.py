"""Surface smoothing (tssplat_amd/smooth.py; tsamd_smooth_*): Taubin's filter and tangential relaxation on the umbrella operator.  The
statement is tests/smooth_oracle.py; the device results are compared with it on bytes: the adjacency, the vertices and the four counts.
The oracle itself is checked on the CPU against hand-worked meshes in Python fractions and against what smoothing is known to do."""
import ctypes as C
import functools
import hashlib
import inspect
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import quality_oracle as QO
import smooth_oracle as SO
from tssplat_amd import _build, _capi, smooth

gpu = pytest.mark.gpu
INVALID = 1     # TSAMD_ERR_INVALID_ARGUMENT
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
MODES = ("taubin", "tangential")
ADJ_FIELDS = ("offsets", "neighbours", "face_offsets", "faces_of", "irregular", "valid")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------- meshes ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden(name):
    d = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    return np.ascontiguousarray(d["vertices"], dtype=F32), np.ascontiguousarray(d["faces"], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def _noisy_sphere():
    v, f = _golden("s1_sphere")
    s = 1 + 0.02 * np.random.default_rng(0).standard_normal(v.shape[0])
    return (v.astype(np.float64) * s[:, None]).astype(F32), f


TET_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F32)
TET = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int32)                       # outward
OCT_V = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F32)
OCT = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)   # outward


def _grid_patch():
    """3 x 3 vertices, vertex 3 i + j at (i, j, 0) but for the centre, every cell cut along its a - c diagonal: eight triangles, open."""
    v = np.array([[i, j, 0] for i in range(3) for j in range(3)], F32)
    v[4] = [1.25, 0.75, 0.5]
    f = []
    for i in range(2):
        for j in range(2):
            a, b, c, d = 3 * i + j, 3 * (i + 1) + j, 3 * (i + 1) + j + 1, 3 * i + j + 1
            f += [[a, b, c], [a, c, d]]
    return v, np.asarray(f, np.int32)


GRID_ROWS = [[1, 3, 4], [0, 2, 4, 5], [1, 5], [0, 4, 6, 7], [0, 1, 3, 5, 7, 8], [1, 2, 4, 8], [3, 7], [3, 4, 6, 8], [4, 5, 7]]     # worked by hand from the eight faces
GRID_FACES_OF_4 = [0, 1, 2, 5, 6, 7]


def _bipyramid(nv, seed=0):
    """A closed strip around two apexes: vertices 0 and 1, a ring of nv - 2; 2 (nv - 2) triangles, every edge in two of them (nv >= 5).  The
    apexes are hubs of degree nv - 2 next to ring vertices of degree 4.  nv = 1: one vertex and a face that names it three times (invalid);
    nv = 3: one triangle listed in both directions; nv = 4: the tetrahedron."""
    rng = np.random.default_rng(seed + nv)
    if nv == 1:
        return rng.standard_normal((1, 3)).astype(F32), np.zeros((1, 3), np.int32)
    if nv == 3:
        return rng.standard_normal((3, 3)).astype(F32), np.array([[0, 1, 2], [0, 2, 1]], np.int32)
    if nv == 4:
        return (TET_V + 0.1 * rng.standard_normal((4, 3))).astype(F32), TET
    n = nv - 2
    a = 2 * np.pi * np.arange(n) / n
    r = 1 + 0.2 * rng.standard_normal(n)
    ring = np.stack([r * np.cos(a), r * np.sin(a), 0.1 * rng.standard_normal(n)], 1)
    v = np.concatenate([[[0.1, 0, 0.8], [0, -0.1, -0.7]], ring]).astype(F32)
    k = np.arange(n)
    k1 = (k + 1) % n
    f = np.concatenate([np.stack([0 * k, 2 + k, 2 + k1], 1), np.stack([0 * k + 1, 2 + k1, 2 + k], 1)])
    return v, f.astype(np.int32)


def _fan(degree=300):
    """An open fan: hub 0, rim 1 .. degree; the rim's two ends have degree 2, the others 3."""
    rng = np.random.default_rng(degree)
    a = 1.5 * np.pi * np.arange(degree) / degree
    r = 1 + 0.1 * rng.standard_normal(degree)
    v = np.concatenate([[[0.05, -0.02, 0.4]], np.stack([r * np.cos(a), r * np.sin(a), 0.05 * rng.standard_normal(degree)], 1)]).astype(F32)
    k = np.arange(1, degree)
    return v, np.stack([0 * k, k, k + 1], 1).astype(np.int32)


def _bow_tie():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]], F32)
    return v, np.concatenate([TET, np.array([0, 4, 5, 6])[TET][:, ::-1]]).astype(np.int32)


def _edge_tets():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, -1, 0], [0, 0, -1]], F32)
    return v, np.concatenate([TET, np.array([0, 1, 4, 5])[TET]]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _hostile():
    """One mesh with everything in it.  Parts, each with its own vertices: a closed bipyramid (11 vertices) with one NaN and one inf vertex
    and one face listed twice; the open 3 x 3 patch; the bow-tie; two tetrahedra sharing an edge; two unreferenced vertices (one of them
    NaN).  Then faces with an index past the end, a negative index and a repeated index, all on bipyramid vertices."""
    parts = [_bipyramid(11, 5), _grid_patch(), _bow_tie(), _edge_tets()]
    vs, fs, base = [], [], 0
    for v, f in parts:
        vs.append(v + F32(0.01) * np.arange(3, dtype=F32) * F32(base))
        fs.append(f + base)
        base += v.shape[0]
    v = np.concatenate(vs + [np.array([[5, 5, 5], [np.nan, 0, 0]], F32)]).astype(F32)
    v[4] = [0.3, np.nan, 0.1]
    v[8, 2] = np.inf
    f = np.concatenate(fs + [fs[0][3:4], [[0, 2, v.shape[0]], [1, -1, 3], [2, 2, 5], [6, 7, 6]]]).astype(np.int32)
    return v, f


def _mesh(name):
    if name in ("s1_sphere", "mario_mesh"):
        return _golden(name)
    return {"tet": lambda: (TET_V, TET), "oct": lambda: (OCT_V, OCT), "grid": _grid_patch, "fan": _fan, "hostile": _hostile, "bow_tie": _bow_tie,
            "edge_tets": _edge_tets, "noisy": _noisy_sphere}[name]()


@functools.lru_cache(maxsize=None)
def _oracle(name, iterations=10, mode="taubin", lam=0.5, mu=-0.53, boundary="fixed", max_move=None):
    """Computed once per (mesh, setting) and shared; the arrays are not to be written to."""
    v, f = _mesh(name)
    return SO.smooth(v, f, iterations, mode, lam, mu, boundary, None, max_move)


# ---------------------------------------------------------------- CPU: the oracle against hand-worked values ----------------------------------------------------------------
def _rows(adj):
    return [adj["neighbours"][adj["offsets"][i]:adj["offsets"][i + 1]].tolist() for i in range(adj["offsets"].size - 1)]


def _fr(x):
    return [Fraction(float(c)) for c in x]


def _frac_step(v, row, coef, faces=None):
    """One half-step of one vertex in exact rationals: (taubin, tangential or None)."""
    p = _fr(v[row[0]])
    nb = [_fr(v[j]) for j in row[1]]
    L = [sum(q[c] for q in nb) / len(nb) - p[c] for c in range(3)]
    d = [Fraction(coef) * x for x in L]
    taubin = [p[c] + d[c] for c in range(3)]
    if faces is None:
        return taubin, None
    n = [Fraction(0)] * 3
    for a, b, c in faces:
        A, B, Cc = _fr(v[a]), _fr(v[b]), _fr(v[c])
        u, w = [B[k] - A[k] for k in range(3)], [Cc[k] - A[k] for k in range(3)]
        n = [n[0] + u[1] * w[2] - u[2] * w[1], n[1] + u[2] * w[0] - u[0] * w[2], n[2] + u[0] * w[1] - u[1] * w[0]]
    s = sum(d[k] * n[k] for k in range(3)) / sum(x * x for x in n)
    return taubin, [p[k] + d[k] - n[k] * s for k in range(3)]


def _close(got, want):
    """A handful of float64 roundings of numbers of magnitude one against the exact rational."""
    return all(abs(Fraction(float(g)) - w) <= Fraction(1, 2 ** 48) for g, w in zip(got, want))


def test_tetrahedron_by_hand():
    adj = SO.adjacency(TET, 4)
    assert _rows(adj) == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]] and adj["irregular"].tolist() == [0] * 4 and adj["valid"].tolist() == [1] * 4
    assert adj["face_offsets"].tolist() == [0, 3, 6, 9, 12] and adj["faces_of"].tolist() == [0, 1, 3, 0, 1, 2, 0, 2, 3, 1, 2, 3]
    move = np.ones(4, bool)
    p = SO.half_step(TET_V.astype(np.float64), TET, adj, move, "taubin", 0.5)
    # vertex 0: the mean of the others is (1/3, 1/3, 1/3), half of it is (1/6, 1/6, 1/6); vertex 1: (1, 0, 0) + ((0, 1/3, 1/3) - (1, 0, 0)) / 2
    assert p[0].tolist() == [float(Fraction(1, 6))] * 3 and p[1].tolist() == [0.5, float(Fraction(1, 6)), float(Fraction(1, 6))]
    for i in range(4):
        faces = TET[[t for t in range(4) if i in TET[t]]]
        taubin, tang = _frac_step(TET_V, (i, _rows(adj)[i]), Fraction(1, 2), faces)
        assert _close(p[i], taubin)
        assert _close(SO.half_step(TET_V.astype(np.float64), TET, adj, move, "tangential", 0.5)[i], tang)


def test_octahedron_by_hand():
    adj = SO.adjacency(OCT, 6)
    assert _rows(adj) == [[2, 3, 4, 5], [2, 3, 4, 5], [0, 1, 4, 5], [0, 1, 4, 5], [0, 1, 2, 3], [0, 1, 2, 3]]
    assert adj["irregular"].tolist() == [0] * 6 and np.diff(adj["face_offsets"]).tolist() == [4] * 6
    assert adj["faces_of"][:4].tolist() == [0, 3, 4, 7]                      # the faces that name vertex 0, ascending
    move = np.ones(6, bool)
    p = SO.half_step(OCT_V.astype(np.float64), OCT, adj, move, "taubin", 0.5)
    assert p.tolist() == (OCT_V * 0.5).tolist()                              # every umbrella points at the centre: L = -p
    # the normal at a vertex is along the vertex: the whole displacement is normal, and tangential relaxation leaves the octahedron alone
    n = SO.vertex_normals(OCT_V.astype(np.float64), OCT, adj)
    assert n.tolist() == (OCT_V * 4.0).tolist()
    q = SO.half_step(OCT_V.astype(np.float64), OCT, adj, move, "tangential", 0.5)
    assert q.tolist() == OCT_V.tolist()
    # a face listed twice: its three edges are in three faces each, so its corners are irregular; a lone triangle in both directions is regular
    assert SO.adjacency(np.concatenate([OCT, OCT[:1]]), 6)["irregular"].tolist() == [1, 0, 1, 0, 1, 0]
    assert SO.adjacency(np.array([[0, 1, 2], [0, 2, 1]]), 3)["irregular"].tolist() == [0, 0, 0]


def test_grid_patch_by_hand():
    v, f = _grid_patch()
    adj = SO.adjacency(f, 9)
    assert _rows(adj) == GRID_ROWS and adj["irregular"].tolist() == [1, 1, 1, 1, 0, 1, 1, 1, 1]
    assert adj["faces_of"][adj["face_offsets"][4]:adj["face_offsets"][5]].tolist() == GRID_FACES_OF_4
    got = SO.smooth(v, f, 1, "taubin", 0.5, 0.0)
    assert (got["moved"], got["held_other"], got["held_pinned"], got["held_irregular"]) == (1, 0, 0, 8)
    # the centre (1.25, 0.75, 0.5): its six neighbours' mean is (1, 1, 0), L = (-0.25, 0.25, -0.5), all exact in binary
    assert got["v"][4].tolist() == [1.125, 0.875, 0.25] and got["v"][[0, 1, 2, 3, 5, 6, 7, 8]].tobytes() == v[[0, 1, 2, 3, 5, 6, 7, 8]].tobytes()
    taubin, tang = _frac_step(v, (4, GRID_ROWS[4]), Fraction(1, 2), f[GRID_FACES_OF_4])
    assert taubin == [Fraction(9, 8), Fraction(7, 8), Fraction(1, 4)]
    assert _close(SO.smooth(v, f, 1, "tangential")["state"][4], tang)
    # with the border free every vertex moves, each to its own row's mean
    free = SO.smooth(v, f, 1, "taubin", 0.5, 0.0, boundary="free")
    assert free["moved"] == 9
    for i in range(9):
        assert _close(free["state"][i], _frac_step(v, (i, GRID_ROWS[i]), Fraction(1, 2))[0])
    # a pinned centre is counted as pinned; a pinned border vertex too, because pinned comes before irregular
    pin = np.zeros(9, bool)
    pin[[4, 0]] = True
    held = SO.smooth(v, f, 3, pinned=pin)
    assert (held["moved"], held["held_pinned"], held["held_irregular"]) == (0, 2, 7) and held["v"].tobytes() == v.tobytes()


def test_hostile_mesh_classification():
    v, f = _hostile()
    adj = SO.adjacency(f, v.shape[0])
    assert adj["valid"][-4:].tolist() == [0, 0, 0, 0] and adj["valid"][:-4].all()
    cls = SO.classify(v, adj)
    nv = v.shape[0]
    assert cls[nv - 2:].tolist() == [1, 1] and cls[4] == 1 and cls[8] == 1          # unreferenced (one of them NaN), the NaN and the inf vertex
    nb = lambda i: adj["neighbours"][adj["offsets"][i]:adj["offsets"][i + 1]]     # noqa: E731
    assert all(cls[j] == 1 for j in nb(4)) and all(cls[j] == 1 for j in nb(8))      # ... and their neighbours
    dup = f[3]                                                                     # listed twice: three faces at each of its edges
    assert all(adj["irregular"][j] for j in dup)
    assert all(cls[11 + i] == 3 for i in (0, 1, 2, 3, 5, 6, 7, 8)) and cls[11 + 4] == 0     # the open patch: the border is held, the centre moves
    assert (cls[20:27] == 0).all()                                                 # the bow-tie's edges are all in two faces: every vertex moves
    assert cls[27:33].tolist() == [3, 3, 0, 0, 0, 0]                                # the shared edge's two ends
    got = SO.smooth(v, f, 2, "tangential")
    assert got["v"].view(np.uint32)[cls != 0].tobytes() == v.view(np.uint32)[cls != 0].tobytes()
    assert np.isfinite(got["v"][cls == 0]).all() and (got["v"][cls == 0] != v[cls == 0]).any() and cls[2] == cls[10] == 0
    assert SO.smooth(v, f, 2, boundary="free")["held_irregular"] == 0


# ---------------------------------------------------------------- CPU: the oracle against what smoothing is known to do ----------------------------------------------------------------
def _radius(v):
    return np.linalg.norm(v.astype(np.float64), axis=1)


def test_taubin_halves_the_noise_and_keeps_the_radius():
    v, _ = _noisy_sphere()
    r0, r1 = _radius(v), _radius(_oracle("noisy")["v"])
    print(f"radius std {r0.std():.4f} -> {r1.std():.4f}, mean {r0.mean():.4f} -> {r1.mean():.4f}")
    assert abs(r0.std() - 0.0198) < 1e-4                                     # the mesh the figures were stated for
    assert r1.std() <= 0.5 * r0.std() and abs(r1.mean() - r0.mean()) < 0.005


def test_plain_laplacian_shrinks():
    r1 = _radius(_oracle("noisy", mu=0.0)["v"])
    print(f"mu = 0: radius std {r1.std():.4f}, mean {r1.mean():.4f}")
    assert r1.mean() < 0.98


def test_tangential_improves_triangles_and_keeps_the_volume():
    v, f = _golden("s1_sphere")
    out = _oracle("s1_sphere", mode="tangential")["v"]
    a0, a1, vol0, vol1 = SO.alr(v, f).min(), SO.alr(out, f).min(), SO.volume(v, f), SO.volume(out, f)
    print(f"min ALR {a0:.4f} -> {a1:.4f}, volume {vol0:.6f} -> {vol1:.6f}")
    assert a1 > 0.9 and abs(vol1 - vol0) < 1e-4 * abs(vol0)


def test_exactly_the_vertices_on_a_non_two_edge_of_mario_keep_their_bits():
    v, f = _golden("mario_mesh")
    got = _oracle("mario_mesh", mode="tangential")
    # the oracle's own edge count
    a, b = f.astype(np.int64).reshape(-1), f[:, [1, 2, 0]].astype(np.int64).reshape(-1)
    und = (np.minimum(a, b) << 32) | np.maximum(a, b)
    keys, counts = np.unique(und, return_counts=True)
    odd = keys[counts != 2]
    on_edge = np.zeros(v.shape[0], bool)
    on_edge[odd >> 32] = True
    on_edge[odd & 0xFFFFFFFF] = True
    # quality_oracle's boundary and non-manifold edges are those edges
    topo = QO.topology(f, v.shape[0])
    assert odd.size == topo["boundary_edges"] + topo["nonmanifold_edges"] == 125 + 170
    same = (got["v"].view(np.uint32) == v.view(np.uint32)).all(1)
    assert np.array_equal(same, on_edge) and int(on_edge.sum()) == got["held_irregular"] == 299
    assert (got["moved"], got["held_other"], got["held_pinned"]) == (v.shape[0] - 299, 0, 0)
    assert np.array_equal(SO.adjacency(f, v.shape[0])["irregular"] != 0, on_edge)


# ---------------------------------------------------------------- CPU: plumbing and argument checks ----------------------------------------------------------------
def test_build_lists_signatures_and_defaults():
    assert {"smooth_kernels.hip", "smooth_capi.cpp"} <= set(_build.SOURCES) and "smooth.h" in _build.HEADERS
    assert _build.SOURCE_FLAGS["smooth_kernels.hip"] == ["-ffp-contract=off"]
    for name in ("smooth_kernels.hip", "smooth_capi.cpp", "smooth.h"):
        assert os.path.exists(os.path.join(_build.CSRC, name))
    names = {"tsamd_smooth_keys", "tsamd_smooth_rows", "tsamd_smooth_classify", "tsamd_smooth_step", "tsamd_smooth_run"}
    assert names <= set(_capi.SIGNATURES)
    header = open(os.path.join(ROOT, "include", "tssplat_amd.h")).read()
    assert all(f" {n}(" in header for n in names)
    assert _capi.ABI_VERSION == 3 and _capi.load().tsamd_abi_version() == 3   # an addition is no incompatible change
    assert C.sizeof(_capi.SmoothMeshStruct) == 8 + 4 * 8 + 5 * 8
    from tssplat_amd import geometry, merge, renderers
    sig = inspect.signature(smooth.smooth).parameters
    assert [(k, p.default) for k, p in sig.items()][2:] == [("iterations", 10), ("mode", "taubin"), ("lam", 0.5), ("mu", -0.53), ("boundary", "fixed"), ("pinned", None),
                                                           ("max_move", None), ("project", False), ("adjacency", None)]
    for fn in (merge.merge_tets, geometry.TetMeshGeometry.export_merged, renderers.MeshRasterizer.export_merged):
        last = list(inspect.signature(fn).parameters.items())[-1]
        assert last[0] == "smooth" and last[1].default is None, fn
    assert "smoothed" in {f.name for f in __import__("dataclasses").fields(merge.MergedSurface)}
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import train_object
    finally:
        sys.path.pop(0)
    assert inspect.signature(train_object.run).parameters["merge_smooth"].default == 0
    assert smooth.MAX_ITERATIONS == SO.MAX_ITERATIONS == 4096 and smooth.STATE_STRIDE in (3, 4)


def _mesh_struct(nv=4, nt=4, nn=12, nf=12, offsets=0x1000, neighbours=0x1000, face_offsets=0x1000, faces_of=0x1000, faces=0x1000, size=None):
    m = _capi.SmoothMeshStruct()
    m.struct_size = C.sizeof(_capi.SmoothMeshStruct) if size is None else size
    m.n_vertices, m.n_triangles, m.n_neighbours, m.n_face_entries = nv, nt, nn, nf
    m.offsets_dev, m.neighbours_dev, m.face_offsets_dev, m.faces_of_dev, m.faces_dev = offsets, neighbours, face_offsets, faces_of, faces
    return m


def test_c_abi_argument_errors_launch_nothing():
    """Every argument error is reported before anything touches the device: all device pointers here are null or made up."""
    lib = _capi.load()
    p, odd = 0x1000, 0x1002                                                 # "not null", aligned / not 4-byte aligned; never dereferenced on these paths
    flag = C.c_int32(7)

    def keys(f=p, nt=4, nv=4, valid=p, ek=p, fk=p):
        return lib.tsamd_smooth_keys(f, nt, nv, valid, ek, fk, None)

    def rows(k=p, n=24, nv=4, head=p, irr=p):
        return lib.tsamd_smooth_rows(k, n, nv, head, irr, None)

    def classify(v=p, irr=p, pinned=None, boundary=0, out=p, mesh=True, **kw):
        return lib.tsamd_smooth_classify(v, C.byref(_mesh_struct(**kw)) if mesh else None, irr, pinned, boundary, out, None)

    def step(src=p, dst=0x2000, stride=4, cls=p, mode=0, coef=0.5, v0=None, r=0.0, mesh=True, **kw):
        return lib.tsamd_smooth_step(src, dst, stride, C.byref(_mesh_struct(**kw)) if mesh else None, cls, mode, coef, v0, r, None)

    def run(a=p, b=0x2000, stride=4, cls=p, mode=0, lam=0.5, mu=-0.53, iterations=1, v0=None, r=0.0, out=True, mesh=True, **kw):
        return lib.tsamd_smooth_run(a, b, stride, C.byref(_mesh_struct(**kw)) if mesh else None, cls, mode, lam, mu, iterations, v0, r,
                                    C.byref(flag) if out else None, None)

    big = 2 ** 31
    cases = [
        (keys, dict(nt=-1), "n_triangles"), (keys, dict(nt=big // 6), "n_triangles"), (keys, dict(nv=-1), "n_vertices"), (keys, dict(nv=big), "n_vertices"),
        (keys, dict(f=None), "faces_dev"), (keys, dict(valid=None), "valid_out_dev"), (keys, dict(ek=None), "edge_keys_out_dev"), (keys, dict(fk=None), "face_keys_out_dev"),
        (keys, dict(f=odd), "faces_dev"), (keys, dict(ek=0x1004), "edge_keys_out_dev"), (keys, dict(fk=0x1004), "face_keys_out_dev"),
        (rows, dict(n=-1), "n_keys"), (rows, dict(n=big), "n_keys"), (rows, dict(nv=big), "n_vertices"), (rows, dict(k=None), "sorted_keys_dev"),
        (rows, dict(k=0x1004), "sorted_keys_dev"), (rows, dict(head=None), "head_out_dev"), (rows, dict(irr=None), "irregular_out_dev"),
        (classify, dict(mesh=False), "mesh is null"), (classify, dict(size=8), "struct_size"), (classify, dict(nv=-1), "n_vertices"), (classify, dict(nt=big), "n_triangles"),
        (classify, dict(nn=-1), "n_neighbours"), (classify, dict(nf=big), "n_face_entries"), (classify, dict(offsets=None), "offsets_dev"),
        (classify, dict(neighbours=odd), "neighbours_dev"), (classify, dict(v=None), "v_dev"), (classify, dict(v=odd), "v_dev"), (classify, dict(irr=None), "irregular_dev"),
        (classify, dict(out=None), "class_out_dev"), (classify, dict(boundary=2), "boundary"),
        (step, dict(stride=2), "stride"), (step, dict(stride=5), "stride"), (step, dict(mode=2), "mode"), (step, dict(mesh=False), "mesh is null"),
        (step, dict(src=None), "src_dev"), (step, dict(dst=None), "dst_dev"), (step, dict(src=0x1008), "src_dev"), (step, dict(dst=0x2010), "dst_dev"),
        (step, dict(stride=3, src=0x1004), "src_dev"), (step, dict(dst=p), "another buffer"), (step, dict(cls=None), "class_dev"),
        (step, dict(v0=p, r=-1.0), "max_move"), (step, dict(v0=p, r=float("nan")), "max_move"), (step, dict(v0=p, r=float("inf")), "max_move"), (step, dict(v0=odd), "v0_dev"),
        (step, dict(mode=1, face_offsets=None), "face_offsets_dev"), (step, dict(mode=1, faces_of=None), "faces_of_dev"), (step, dict(mode=1, faces=odd), "faces_dev"),
        (step, dict(neighbours=None), "neighbours_dev"),
        (run, dict(iterations=-1), "iterations"), (run, dict(iterations=4097), "iterations"), (run, dict(lam=float("nan")), "lam / mu"), (run, dict(out=False), "result_in_b_out"),
        (run, dict(a=None), "state_a_dev"), (run, dict(b=0x2008), "state_b_dev"), (run, dict(b=p), "another buffer"), (run, dict(stride=0), "stride"),
        (run, dict(mode=-1), "mode"), (run, dict(cls=None), "class_dev"), (run, dict(v0=p, r=-0.5), "max_move"), (run, dict(mode=1, faces=None), "faces_dev"),
        (run, dict(nv=big), "n_vertices"),
    ]
    for fn, kw, word in cases:
        assert fn(**kw) == INVALID, (fn.__name__, kw)
        msg = lib.tsamd_last_error().decode()
        assert msg and word in msg, (fn.__name__, kw, msg)
    # nothing to do is not an error, and still launches nothing
    assert keys(nt=0, f=None, valid=None, ek=None, fk=None) == 0
    assert classify(nv=0, nn=0, nf=0, v=None, irr=None, out=None, offsets=None, neighbours=None) == 0
    assert step(nv=0, nn=0, nf=0, src=None, dst=None, cls=None, offsets=None) == 0
    assert run(nv=0, nn=0, nf=0, a=None, b=None, cls=None, offsets=None, iterations=4096) == 0 and flag.value == 0
    assert run(iterations=0) == 0 and flag.value == 0                       # no half-step: the result is where it was
    assert run(iterations=3, lam=0.0, mu=0.0) == 0 and flag.value == 0      # every half-step skipped
    assert step(mode=0, face_offsets=None, faces_of=None, faces=None, nv=0) == 0
    assert _capi.ABI_VERSION == 3 and lib.tsamd_abi_version() == 3


def test_python_arguments_are_checked_by_name():
    """Nothing here reaches the library: a CPU tensor is refused, with the argument's name, after everything that can be said without one."""
    v, f = torch.zeros(4, 3), torch.zeros(1, 3, dtype=torch.int32)
    S = smooth.smooth
    for call, word in [(lambda: S(v, f), "v must be a GPU tensor"), (lambda: S(v, f, iterations=-1), "iterations must be"), (lambda: S(v, f, iterations=4097), "iterations must be"),
                       (lambda: S(v, f, iterations=1.5), "iterations must be"), (lambda: S(v, f, iterations=True), "iterations must be"), (lambda: S(v, f, mode="cotan"), "mode must be"),
                       (lambda: S(v, f, lam=float("nan")), "lam must be"), (lambda: S(v, f, mu=float("inf")), "mu must be"), (lambda: S(v, f, mu="x"), "mu must be"),
                       (lambda: S(v, f, boundary="open"), "boundary must be"), (lambda: S(v, f, max_move=-1.0), "max_move must be"),
                       (lambda: S(v, f, max_move=float("nan")), "max_move must be"), (lambda: S(v, f, project=1), "project must be"), (lambda: S(v.double(), f), "v must be float32"),
                       (lambda: S(v, f.long()), "faces must be int32"), (lambda: S(v[:, :2], f), "v must be"), (lambda: S(None, f), "v must"),
                       (lambda: smooth.adjacency(f, 4), "faces must be a GPU tensor"), (lambda: smooth.adjacency(f.long(), 4), "faces must be int32"),
                       (lambda: smooth.adjacency(f, -1), "n_vertices must be"), (lambda: smooth.adjacency(f, 2.0), "n_vertices must be")]:
        with pytest.raises(RuntimeError, match="tssplat_amd.smooth.*" + word):
            call()
    from tssplat_amd import merge
    for bad in (0, -1, 1.5, True, 4097, "3"):
        with pytest.raises(RuntimeError, match="tssplat_amd.merge.merge_tets: smooth must be"):
            merge.merge_tets(v, torch.zeros(1, 4, dtype=torch.int32), smooth=bad)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="needs the ROCm LLVM tools")
def test_kernels_are_in_the_code_object_and_do_not_spill():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_metadata
    finally:
        sys.path.pop(0)
    _capi.load()
    meta = kernel_metadata.kernel_metadata(_capi.lib_path())
    for want, n in (("smooth_keys_kernel", 1), ("smooth_rows_kernel", 1), ("smooth_classify_kernel", 1), ("smooth_step_kernel", 4)):
        recs = [v for k, v in meta.items() if want in k]
        assert len(recs) == n, want
        for rec in recs:
            assert rec["vgpr_spill_count"] == 0 and rec["private_segment_fixed_size"] == 0 and rec["group_segment_fixed_size"] == 0, (want, rec)


# ---------------------------------------------------------------- GPU: bytes ----------------------------------------------------------------
def _assert_adjacency(f, nv, what):
    want = SO.adjacency(f, nv)
    got = smooth.adjacency(dev(f), nv)
    for key in ADJ_FIELDS:
        g = getattr(got, key)
        assert g.dtype == (torch.uint8 if key in ("irregular", "valid") else torch.int32), (what, key)
        assert g.cpu().numpy().tobytes() == want[key].tobytes(), (what, key)
    return got


def _assert_smooth(v, f, what, want=None, pinned=None, **kw):
    """The vertices and the four counts equal the oracle's bytes; ``faces`` is the caller's tensor."""
    if want is None:
        want = SO.smooth(v, f, pinned=pinned, **{("adj" if k == "adjacency" else k): x for k, x in kw.items() if k != "adjacency"})
    df = dev(f)
    got = smooth.smooth(dev(v), df, pinned=None if pinned is None else dev(pinned), **kw)
    assert got.faces is df and got.v.dtype == torch.float32 and tuple(got.v.shape) == v.shape
    assert got.v.cpu().numpy().tobytes() == want["v"].tobytes(), what
    for key in SO.HELD_NAMES:
        assert getattr(got, key) == want[key] and type(getattr(got, key)) is int, (what, key, getattr(got, key), want[key])
    return got


@gpu
@pytest.mark.parametrize("nv", [1, 3, 4, 63, 64, 65, 129, 130, 131, 255, 256, 257])
def test_every_launch_edge(nv):
    """Vertex counts around one wave and one workgroup; 2 (nv - 2) faces, so nv = 129, 130, 131 put 254, 256 and 258 faces around a workgroup of faces."""
    v, f = _bipyramid(nv)
    _assert_adjacency(f, nv, nv)
    for mode in MODES:
        _assert_smooth(v, f, (nv, mode), iterations=3, mode=mode)


@gpu
def test_a_hub_of_degree_300_next_to_rim_vertices_of_degree_2():
    v, f = _fan(300)
    adj = _assert_adjacency(f, v.shape[0], "fan")
    deg = np.diff(adj.offsets.cpu().numpy())
    assert deg[0] == 300 and deg[1] == deg[300] == 2 and (deg[2:300] == 3).all()
    for mode in MODES:
        got = _assert_smooth(v, f, ("fan free", mode), iterations=3, mode=mode, boundary="free")
        assert got.moved == 301
        got = _assert_smooth(v, f, ("fan fixed", mode), iterations=3, mode=mode)      # every vertex lies on a boundary edge
        assert got.held_irregular == 301 and got.v.cpu().numpy().tobytes() == v.tobytes()


@gpu
def test_hostile_mesh_gets_the_oracles_classes_and_bits():
    v, f = _hostile()
    _assert_adjacency(f, v.shape[0], "hostile")
    for name in ("bow_tie", "edge_tets", "grid"):
        _assert_adjacency(_mesh(name)[1], _mesh(name)[0].shape[0], name)
    pin = np.zeros(v.shape[0], bool)
    pin[[2, 4, 15, 20, 27]] = True                                          # a mover, the NaN vertex (other comes first), the patch's centre, a bow-tie and an irregular vertex
    for mode in MODES:
        for boundary in ("fixed", "free"):
            got = _assert_smooth(v, f, ("hostile", mode, boundary), iterations=2, mode=mode, boundary=boundary)
            assert got.held_other > 0 and (got.held_irregular > 0) == (boundary == "fixed")
            got = _assert_smooth(v, f, ("hostile pinned", mode, boundary), pinned=pin, iterations=2, mode=mode, boundary=boundary)
            assert got.held_pinned == 4
    # pinned as uint8 is the same mask
    a = smooth.smooth(dev(v), dev(f), pinned=dev(pin))
    b = smooth.smooth(dev(v), dev(f), pinned=dev(pin.astype(np.uint8)))
    assert a.v.cpu().numpy().tobytes() == b.v.cpu().numpy().tobytes() and a.held_pinned == b.held_pinned


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_iteration_counts_land_in_the_right_buffer(mode):
    """0, 1, 2, 3 and 10 iterations: one half-step per iteration (tangential, and Taubin with mu = 0) alternates the buffer the result is in."""
    v, f = _noisy_sphere()
    for it in (0, 1, 2, 3, 10):
        got = _assert_smooth(v, f, (mode, it), want=_oracle("noisy", it, mode), iterations=it, mode=mode)
        assert got.iterations == it and got.moved == v.shape[0]
        if mode == "taubin":
            _assert_smooth(v, f, ("mu = 0", it), want=_oracle("noisy", it, mode, mu=0.0), iterations=it, mu=0.0)
            _assert_smooth(v, f, ("lam = 0", it), want=_oracle("noisy", it, mode, lam=0.0), iterations=it, lam=0.0)
    zero = smooth.smooth(dev(v), dev(f), iterations=0)
    assert zero.v.cpu().numpy().tobytes() == v.tobytes() and zero.moved == v.shape[0]


@gpu
def test_option_combinations():
    v, f = _golden("mario_mesh")
    free = _assert_smooth(v, f, "free", want=_oracle("mario_mesh", 3, "tangential", boundary="free"), iterations=3, mode="tangential", boundary="free")
    assert free.moved == v.shape[0]
    pin = np.zeros(v.shape[0], bool)
    pin[::7] = True
    got = _assert_smooth(v, f, "pinned", pinned=pin, iterations=3)
    assert got.held_pinned > 0 and got.v.cpu().numpy()[::7].tobytes() == v[::7].tobytes()
    # max_move: at 0 nothing changes its value; at the median displacement of the unclamped run it binds on some vertices only
    unclamped = _oracle("mario_mesh", 3)
    move = np.abs(unclamped["state"] - v.astype(np.float64)).max(1)
    r = float(np.median(move[unclamped["cls"] == 0]))
    for mode in MODES:
        at0 = _assert_smooth(v, f, ("max_move 0", mode), iterations=3, mode=mode, max_move=0.0)
        assert np.array_equal(at0.v.cpu().numpy(), v)
        _assert_smooth(v, f, ("max_move None", mode), want=_oracle("mario_mesh", 3, mode), iterations=3, mode=mode, max_move=None)
        want = _oracle("mario_mesh", 3, mode, max_move=r)
        got = _assert_smooth(v, f, ("max_move r", mode), want=want, iterations=3, mode=mode, max_move=r)
        d = np.abs(got.v.cpu().numpy().astype(np.float64) - v.astype(np.float64)).max(1)
        assert d.max() <= r + 2.0 ** -23 * np.abs(v).max() and (want["v"] != _oracle("mario_mesh", 3, mode)["v"]).any()      # r, and the final rounding to float32
        assert got.max_move == r
    binds = np.abs(_oracle("mario_mesh", 3, max_move=r)["state"] - v.astype(np.float64)).max(1) >= r * (1 - 1e-12)
    assert 0 < binds.sum() < (unclamped["cls"] == 0).sum()
    # an adjacency handed back: the same bytes as without
    adj = smooth.adjacency(dev(f), v.shape[0])
    for mode in MODES:
        got = smooth.smooth(dev(v), dev(f), iterations=3, mode=mode, adjacency=adj)
        assert got.v.cpu().numpy().tobytes() == _oracle("mario_mesh", 3, mode)["v"].tobytes() and got.held_irregular == 299
    with pytest.raises(RuntimeError, match="tssplat_amd.smooth.smooth: adjacency.offsets must have shape"):
        smooth.smooth(dev(v[:-1]), dev(f), adjacency=adj)
    with pytest.raises(RuntimeError, match="tssplat_amd.smooth.smooth: pinned must have shape"):
        smooth.smooth(dev(v), dev(f), pinned=dev(pin[:-1]))
    # both state layouts hold the same numbers
    vv, ff = dev(v), dev(f)
    a3 = smooth._smooth("smooth", vv, ff, 3, "tangential", 0.5, -0.53, "fixed", None, None, False, adj, stride=3)
    a4 = smooth._smooth("smooth", vv, ff, 3, "tangential", 0.5, -0.53, "fixed", None, None, False, adj, stride=4)
    assert a3[0].cpu().numpy().tobytes() == a4[0].cpu().numpy().tobytes() == _oracle("mario_mesh", 3, "tangential")["v"].tobytes() and a3[1] == a4[1]


@gpu
@pytest.mark.parametrize("name", ["s1_sphere", "mario_mesh"])
@pytest.mark.parametrize("mode", MODES)
def test_fixtures_equal_oracle_and_repeat(name, mode):
    v, f = _golden(name)
    digests = set()
    for run in range(2):
        got = _assert_smooth(v, f, (name, mode, run), want=_oracle(name, 10, mode), iterations=10, mode=mode)
        digests.add(hashlib.sha256(got.v.cpu().numpy().tobytes()).hexdigest())
    assert len(digests) == 1
    assert (got.mode, got.lam, got.mu, got.boundary, got.max_move, got.project) == (mode, 0.5, -0.53, "fixed", None, False)
    assert got.held_irregular == (299 if name == "mario_mesh" else 0)


@gpu
def test_one_half_step_through_the_c_abi_in_both_layouts():
    """tsamd_smooth_step on its own: the destination equals the oracle's half-step in every record, held vertices included, and the source is untouched."""
    from tssplat_amd import _args
    v, f = _hostile()
    nv = v.shape[0]
    adj = smooth.adjacency(dev(f), nv)
    dv, df = dev(v), dev(f)
    mesh = smooth._mesh_struct(adj, df, nv)
    cls = smooth._classify(dv, mesh, adj, None, "fixed")
    oadj = SO.adjacency(f, nv)
    ocls = SO.classify(v, oadj)
    assert cls.cpu().numpy().tobytes() == ocls.tobytes()
    lib, ctx, stream = _args.lib_and_stream(dv.device)
    p0 = v.astype(np.float64)
    for stride in (3, 4):
        for mode in MODES:
            src = torch.zeros((nv, stride), dtype=torch.float64, device="cuda")
            src[:, :3] = dv.double()
            before = src.clone()
            dst = torch.full_like(src, 7.0)
            with ctx:
                _capi.check(lib.tsamd_smooth_step(src.data_ptr(), dst.data_ptr(), stride, C.byref(mesh), cls.data_ptr(), smooth.MODES[mode], 0.5, dv.data_ptr(), 0.05,
                                                  stream))
            want = SO.half_step(p0, f, oadj, ocls == 0, mode, 0.5, p0, 0.05)
            assert dst[:, :3].contiguous().cpu().numpy().tobytes() == want.tobytes(), (stride, mode)
            assert torch.equal(src.view(torch.int64), before.view(torch.int64)) and (stride == 3 or bool((dst[:, 3] == 0).all()))


@gpu
def test_project_puts_the_moved_vertices_back_on_the_input_surface():
    from tssplat_amd import metrics
    v, f = _golden("s1_sphere")
    dv, df = dev(v), dev(f)
    plain = smooth.smooth(dv, df, mode="tangential")
    got = smooth.smooth(dv, df, mode="tangential", project=True)
    assert got.project is True and got.moved == plain.moved == v.shape[0]
    d2, tri, point = metrics.nearest_on_mesh(plain.v, dv, df)
    assert got.v.cpu().numpy().tobytes() == point.cpu().numpy().tobytes()
    assert plain.v.cpu().numpy().tobytes() == _oracle("s1_sphere", 10, "tangential")["v"].tobytes()
    # The projected vertex is a point of a triangle in float64, rounded to float32 coordinate by coordinate.  The sphere's coordinates
    # are below 2 in magnitude, where float32 numbers are at most 2^-23 apart (2^-24 below 1, "a coordinate of magnitude 1"), so each
    # coordinate is off by at most half of that, 2^-24, and the squared distance to the triangle, and so to the mesh, by at most
    # 3 (2^-24)^2; the float64 rounding of the closest point itself is eight orders of magnitude below that.
    assert np.abs(v).max() < 2
    back = metrics.nearest_on_mesh(got.v, dv, df)[0].cpu().numpy().astype(np.float64)
    print(f"squared distance to the input after projection: max {back.max():.3e}, bound {3 * (2.0 ** -24) ** 2:.3e}; before: {float(d2.max()):.3e}")
    assert back.max() <= 3 * (2.0 ** -24) ** 2
    assert float(d2.max()) > 3 * (2.0 ** -24) ** 2                           # the unprojected vertices had left the surface
    # nothing to project onto is an argument error
    for vv, ff in ((np.full_like(v, np.nan), f), (v, f + v.shape[0]), (v, f[:0]), (v[:0], f)):
        with pytest.raises(RuntimeError, match="tssplat_amd.smooth.smooth: project=True needs a valid triangle"):
            smooth.smooth(dev(vv), dev(ff), project=True)


@gpu
def test_empty_inputs_return_without_a_device_call():
    v, f = _golden("s1_sphere")
    got = smooth.smooth(dev(v), dev(f[:0]))
    assert got.v.cpu().numpy().tobytes() == v.tobytes() and (got.moved, got.held_other, got.held_pinned, got.held_irregular) == (0, v.shape[0], 0, 0)
    got = smooth.smooth(dev(v[:0]), dev(f))
    assert tuple(got.v.shape) == (0, 3) and (got.moved, got.held_other) == (0, 0)
    adj = smooth.adjacency(dev(f[:0]), 5)
    assert adj.offsets.tolist() == [0] * 6 and adj.neighbours.numel() == 0 and adj.irregular.tolist() == [0] * 5 and adj.valid.numel() == 0
    _assert_adjacency(f + v.shape[0], v.shape[0], "all invalid")
    got = _assert_smooth(v, f + v.shape[0], "all invalid", iterations=2)
    assert got.held_other == v.shape[0]


@gpu
def test_merge_pipeline(tmp_path):
    from tssplat_amd import geometry, merge, scenes
    bv, bt = scenes.kuhn_ball(2)
    bv = bv / np.linalg.norm(bv, axis=1).max()
    v = np.concatenate([bv * 0.4 + np.asarray([-0.2, 0.05, 0.0]), bv * 0.35 + np.asarray([0.25, -0.1, 0.1])]).astype(F32)     # the scene of test_merge.py
    e = np.concatenate([bt, bt + bv.shape[0]]).astype(np.int32)
    plain = merge.merge_tets(dev(v), dev(e), grid=32)
    want = smooth.smooth(plain.v, plain.faces, iterations=3)
    got = merge.merge_tets(dev(v), dev(e), grid=32, smooth=3)
    assert plain.smoothed is None and isinstance(got.smoothed, smooth.SmoothedSurface) and got.smoothed.iterations == 3 and got.v is got.smoothed.v
    assert got.v.cpu().numpy().tobytes() == want.v.cpu().numpy().tobytes() != plain.v.cpu().numpy().tobytes()
    assert got.faces.cpu().numpy().tobytes() == plain.faces.cpu().numpy().tobytes() and got.closed is plain.closed is True
    assert want.v.cpu().numpy().tobytes() == SO.smooth(plain.v.cpu().numpy(), plain.faces.cpu().numpy(), 3)["v"].tobytes()
    assert got.smoothed.held_other == 0 and got.smoothed.moved + got.smoothed.held_irregular == int(plain.v.shape[0]) and got.smoothed.moved > 0
    both = merge.merge_tets(dev(v), dev(e), grid=32, fill="cavities", simplify=2, smooth=3)
    ref = merge.merge_tets(dev(v), dev(e), grid=32, fill="cavities", simplify=2)
    assert both.v.cpu().numpy().tobytes() == smooth.smooth(ref.v, ref.faces, iterations=3).v.cpu().numpy().tobytes() and both.closed is ref.closed
    geo = geometry.TetMeshGeometry(v, e, use_smooth_barrier=False)
    merged = geo.export_merged(str(tmp_path), "s", grid=32, smooth=3)
    rv = np.asarray([[float(x) for x in ln.split()[1:4]] for ln in open(tmp_path / "s_merged.obj") if ln.startswith("v ")], F32)
    assert rv.tobytes() == merged.v.cpu().numpy().tobytes() == got.v.cpu().numpy().tobytes()
