"""Mesh quality (tssplat_amd/quality.py; tsamd_quality_*): the exact self-intersection search and the topology counts.  The statement
is tests/quality_oracle.py; the device results are compared with it on bytes: crossings, sorted pairs, stats, component and fans.
The oracle itself is checked on the CPU against Python integers, a hand-made table of contacts and meshes whose topology is known."""
import ctypes as C
import dataclasses
import functools
import inspect
import itertools
import os

import numpy as np
import pytest
import torch

import quality_oracle as QO
from tssplat_amd import _build, _capi

gpu = pytest.mark.gpu
INVALID = 1     # TSAMD_ERR_INVALID_ARGUMENT
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
M = QO.LATTICE - 1
UNITY = (0.0, float(M))          # g = 1: an integer coordinate is its own lattice coordinate


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------- meshes ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden(name):
    d = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    return np.ascontiguousarray(d["vertices"], dtype=F32), np.ascontiguousarray(d["faces"], dtype=np.int32)


def _soup(tris):
    """Triangles given corner by corner -> (v, faces) without shared vertices."""
    t = np.asarray(tris, F32).reshape(-1, 3, 3)
    return t.reshape(-1, 3), np.arange(3 * t.shape[0], dtype=np.int32).reshape(-1, 3)


A0 = [(0, 0, 0), (8, 0, 0), (0, 8, 0)]
# (name, second triangle, expected crossing pairs with A0)
TABLE = [
    ("transversal", [(2, 2, -4), (3, 2, 4), (2, 3, 4)], 1),
    ("shared vertex, apart", [(0, 0, 0), (-4, 0, 4), (0, -4, 4)], 0),
    ("shared vertex, opposite edge pierces", [(0, 0, 0), (2, 2, -4), (3, 2, 4)], 1),
    ("shared edge, folded flat", [(0, 0, 0), (8, 0, 0), (2, 6, 0)], 0),
    ("vertex touches the interior", [(2, 2, 0), (2, 2, 8), (3, 3, 8)], 0),
    ("edges through edges (the stated limit)", [(2, 2, 4), (6, -2, -4), (-2, 6, -4)], 0),
    ("coplanar overlap", [(1, 1, 0), (9, 1, 0), (1, 9, 0)], 0),
    ("apart", [(20, 20, 5), (28, 20, 5), (20, 28, 9)], 0),
]


def _table_case(second):
    return _soup(np.asarray([A0, second], np.float64) + 100.0)


def _hostile():
    """0 and 1 cross.  2: degenerate after the snap, through 0's interior.  3: a NaN vertex.  4: a vertex below the cube.  5: above it.
    6: an index past the end.  7: a negative index.  8: repeated index (degenerate)."""
    v, f = _soup(np.asarray([A0, TABLE[0][1], [(2, 2, 0), (2.2, 2, 0), (2, 2.3, 0)], A0, A0, A0], np.float64) + 100.0)
    v[9] = [np.nan, 100, 100]
    v[12] = [-1, 100, 100]
    v[15] = [100, float(M) + 1, 100]
    f = np.concatenate([f, [[0, 1, 18], [0, -1, 2], [3, 3, 4]]]).astype(np.int32)
    return v, f


def _cell_triangle(cell):
    x, y = 8.0 * (cell % 64), 8.0 * (cell // 64)
    return [(x, y, 8), (x + 4, y, 8), (x, y + 4, 8)]


def _cell_needle(cell):
    x, y = 8.0 * (cell % 64), 8.0 * (cell // 64)
    return [(x + 1, y + 1, 6), (x + 2, y + 1, 10), (x + 1, y + 2, 10)]


def _planted(T, partners, target=None):
    """T triangles, one per cell of the plane z = 8, apart from each other; the triangles at the indices ``partners`` (those below T) are
    copies of one needle through the target's triangle.  Expected: one crossing pair per copy, the copies cross nothing else."""
    target = T // 2 if target is None else target
    partners = sorted({p for p in partners if 0 <= p < T and p != target})
    tris = [_cell_needle(target) if t in partners else _cell_triangle(t) for t in range(T)]
    pairs = sorted((min(p, target) << 32) | max(p, target) for p in partners)
    return _soup(tris) + (np.asarray(pairs, np.int64),)


def _drain(copies=200):
    """``copies`` of a triangle and of a needle through it, interleaved: copies^2 crossing pairs, every pair of boxes overlaps."""
    return _soup([_cell_needle(3) if t & 1 else _cell_triangle(3) for t in range(2 * copies)])


def _shifted_spheres():
    v, f = _golden("s1_sphere")
    v2 = (v + np.asarray([0.37, 0.11, 0.05], F32)).astype(F32)
    return np.concatenate([v, v2]), np.concatenate([f, f + v.shape[0]]).astype(np.int32)


def _tight(v):
    return float(np.float64(v.min()) - 1e-3), float(np.float64(v.max()) + 1e-3)


TET = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int32)     # outward for vertices 0 (0,0,0), 1 (1,0,0), 2 (0,1,0), 3 (0,0,1)


def _bow_tie():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]], F32)
    remap = np.array([0, 4, 5, 6])
    return v, np.concatenate([TET, remap[TET][:, ::-1]]).astype(np.int32)


def _edge_tets():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, -1, 0], [0, 0, -1]], F32)
    remap = np.array([0, 1, 4, 5])
    return v, np.concatenate([TET, remap[TET]]).astype(np.int32)


def _moebius(n=9):
    a = 2 * np.pi * np.arange(n) / n
    mid = np.stack([np.cos(a), np.sin(a), 0 * a], 1)
    off = 0.3 * np.stack([np.cos(a / 2) * np.cos(a), np.cos(a / 2) * np.sin(a), np.sin(a / 2)], 1)
    v = np.concatenate([mid + off, mid - off]).astype(F32)                 # top i, bottom n + i
    f = []
    for i in range(n):
        t0, b0 = i, n + i
        t1, b1 = (i + 1, n + i + 1) if i + 1 < n else (n, 0)               # the twist: top meets bottom
        f += [[t0, b0, t1], [t1, b0, b1]]
    return v, np.asarray(f, np.int32)


def _flipped_sphere():
    v, f = _golden("s1_sphere")
    f = f.copy()
    f[17] = f[17, ::-1]
    return v, f


def _two_spheres():
    v, f = _golden("s1_sphere")
    return np.concatenate([v, v + np.asarray([5, 0, 0], F32)]).astype(F32), np.concatenate([f, f + v.shape[0]]).astype(np.int32)


def _unreferenced():
    v, f = _bow_tie()
    return np.concatenate([np.full((2, 3), 9, F32), v, np.full((1, 3), np.nan, F32)]), (f + 2).astype(np.int32)


TOPOLOGY_MESHES = {"s1_sphere": lambda: _golden("s1_sphere"), "mario": lambda: _golden("mario_mesh"), "two_spheres": _two_spheres, "bow_tie": _bow_tie,
                   "edge_tets": _edge_tets, "moebius": _moebius, "flipped": _flipped_sphere, "unreferenced": _unreferenced, "hostile": _hostile}


@functools.lru_cache(maxsize=None)
def _topology_oracle(name):
    v, f = TOPOLOGY_MESHES[name]()
    lo, hi = UNITY if name == "hostile" else _tight(v[np.isfinite(v).all(1)])
    state = QO.prepare(v, f, lo, hi)[1]
    return QO.topology(f, v.shape[0], state != QO.INVALID), (lo, hi)


@functools.lru_cache(maxsize=None)
def _pairs_oracle(name):
    v, f, bounds = PAIR_MESHES[name]()
    return QO.self_intersections(v, f, *bounds)


PAIR_MESHES = {
    "s1_sphere": lambda: _golden("s1_sphere") + (_tight(_golden("s1_sphere")[0]),),
    "shifted_spheres": lambda: _shifted_spheres() + (_tight(_shifted_spheres()[0]),),
    "mario": lambda: _golden("mario_mesh") + (_tight(_golden("mario_mesh")[0]),),
    "hostile": lambda: _hostile() + (UNITY,),
    "drain": lambda: _drain() + (UNITY,),
}


# ---------------------------------------------------------------- CPU: the oracle ----------------------------------------------------------------
def test_orient_in_int64_equals_python_integers_at_the_lattice_extremes():
    """All 4096 quadruples of corners of the lattice cube: the largest determinants there are.  The int64 value equals the Python integer,
    and the bound of the kernel's head holds: below 3 2^61, and 2^60 is reached (one term is (2^20 - 1)^3)."""
    corners = np.array(list(itertools.product((0, M), repeat=3)), np.int64)
    quads = np.array(list(itertools.product(range(8), repeat=4)))
    a, b, c, d = (corners[quads[:, k]] for k in range(4))
    got = QO.orient(a, b, c, d)
    want = [QO.orient_exact(*(corners[q] for q in quad)) for quad in quads]
    assert got.tolist() == want
    assert max(abs(x) for x in want) < 3 * 2 ** 61 and max(abs(x) for x in want) >= M ** 3
    rng = np.random.default_rng(0)
    p = rng.integers(0, M + 1, (500, 4, 3))
    assert QO.orient(p[:, 0], p[:, 1], p[:, 2], p[:, 3]).tolist() == [QO.orient_exact(*q) for q in p]


@pytest.mark.parametrize("name,second,expected", TABLE, ids=[t[0] for t in TABLE])
def test_hand_made_contacts(name, second, expected):
    v, f = _table_case(second)
    for faces in (f, f[::-1]):                                              # either triangle first
        got = QO.self_intersections(v, faces, *UNITY)
        assert got["crossing_pairs"] == expected and got["crossing_faces"] == 2 * expected and got["invalid_faces"] == got["degenerate_faces"] == 0
        assert got["pairs"].tolist() == ([1] if expected else []) and got["crossings"].tolist() == [expected, expected]
    # the same contact seen by a mirrored, rotated copy: signs flip, the count does not
    w = v[:, [1, 2, 0]].copy()
    w[:, 0] = 300 - w[:, 0]
    assert QO.self_intersections(w, f, *UNITY)["crossing_pairs"] == expected


def test_edges_through_edges_is_a_real_crossing_that_the_strict_rule_leaves_out():
    """The limit, pinned: the triangles of that table row do cross (moving the second one by one lattice step along an edge shows it)."""
    v, f = _table_case(TABLE[5][1])
    assert QO.self_intersections(v, f, *UNITY)["crossing_pairs"] == 0
    v[3:] += np.asarray([1, 1, 0], F32)
    assert QO.self_intersections(v, f, *UNITY)["crossing_pairs"] == 1


def test_hostile_mesh_states_and_counts():
    v, f = _hostile()
    got = QO.self_intersections(v, f, *UNITY)
    assert got["state"].tolist() == [0, 0, 1, 2, 2, 2, 2, 2, 1]
    assert (got["invalid_faces"], got["degenerate_faces"], got["crossing_pairs"], got["crossing_faces"]) == (5, 2, 1, 2)
    assert got["pairs"].tolist() == [1] and got["crossings"].tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 0]
    corners, state, shape = QO.prepare(v, f, *UNITY)
    assert corners[0].tolist() == [[100, 100, 100], [108, 100, 100], [100, 108, 100]] and (corners[2] == [102, 102, 100]).all()
    assert shape[0].tolist() == [64.0, 128.0, 64.0, 4096.0] and np.isnan(shape[3:8]).all() and np.isfinite(shape[2]).all()
    # the snap: half a lattice step rounds up, and the cube's own corners are inside
    X, ok = QO.snap(np.array([[0, 0.5, 0.49999], [M, M, M], [M + 0.5, 0, 0], [-0.5, 0, 0], [-0.51, 0, 0]], F32), *UNITY)
    assert ok.tolist() == [True, True, False, True, False] and X[0].tolist() == [0, 1, 0] and X[1].tolist() == [M, M, M] and X[3].tolist() == [0, 0, 0]


def test_planted_crossings_are_what_the_oracle_finds():
    v, f, pairs = _planted(40, (0, 7, 39, 99))
    got = QO.self_intersections(v, f, *UNITY)
    assert got["pairs"].tolist() == pairs.tolist() == [(0 << 32) | 20, (7 << 32) | 20, (20 << 32) | 39]
    assert got["crossings"][20] == 3 and got["crossings"].sum() == 6 and got["box_pairs"] == 3 + 3      # the copies' boxes overlap each other too
    v, f = _drain(5)
    got = QO.self_intersections(v, f, *UNITY)
    assert got["crossing_pairs"] == 25 and got["box_pairs"] == 45 and (got["crossings"] == 5).all()


def test_golden_sphere_topology():
    t, _ = _topology_oracle("s1_sphere")
    assert (t["edges"], t["boundary_edges"], t["nonmanifold_edges"], t["repeated_directed_edges"]) == (4494, 0, 0, 0)
    assert t["closed"] and t["oriented"] and t["manifold"] and t["components"] == 1 and t["euler"] == 2 and (t["fans"] == 1).all()
    assert (t["component"] == 0).all()


def test_known_topologies():
    nv = _golden("s1_sphere")[0].shape[0]
    t, _ = _topology_oracle("two_spheres")
    assert t["components"] == 2 and (t["component"][:nv] == 0).all() and (t["component"][nv:] == nv).all() and t["euler"] == 4 and t["closed"]
    t, _ = _topology_oracle("bow_tie")
    assert t["fans"].tolist() == [2, 1, 1, 1, 1, 1, 1] and t["components"] == 1 and t["nonmanifold_vertices"] == 1 and t["nonmanifold_edges"] == 0
    assert t["closed"] and t["oriented"] and not t["manifold"] and t["euler"] == 7 - 12 + 8
    t, _ = _topology_oracle("edge_tets")
    assert t["nonmanifold_edges"] == 1 and t["fans"].tolist() == [1, 1, 1, 1, 1, 1] and t["components"] == 1 and not t["manifold"] and not t["closed"]
    assert t["repeated_directed_edges"] == 2                                # 0 -> 1 twice and 1 -> 0 twice
    t, _ = _topology_oracle("moebius")
    assert not t["oriented"] and t["repeated_directed_edges"] == 1 and t["nonmanifold_edges"] == 0 and t["boundary_edges"] == 18 and t["components"] == 1
    assert (t["fans"] == 1).all() and t["euler"] == 0
    t, _ = _topology_oracle("flipped")
    assert not t["oriented"] and t["repeated_directed_edges"] == 3 and not t["closed"] and t["manifold"] and t["euler"] == 2
    t, _ = _topology_oracle("unreferenced")
    assert t["component"].tolist() == [-1, -1, 2, 2, 2, 2, 2, 2, 2, -1] and t["fans"].tolist() == [0, 0, 2, 1, 1, 1, 1, 1, 1, 0]
    assert t["referenced_vertices"] == 7 and t["components"] == 1
    t, _ = _topology_oracle("hostile")                                      # the valid triangles: 0, 1, 2 and 8
    assert t["valid_faces"] == 4 and t["components"] == 3 and t["referenced_vertices"] == 9


def test_mario_topology_equals_the_prototype():
    t, _ = _topology_oracle("mario")
    assert (t["edges"], t["boundary_edges"], t["nonmanifold_edges"], t["repeated_directed_edges"]) == (11083, 125, 170, 188)
    assert (t["nonmanifold_vertices"], t["euler"], t["components"]) == (6, -3, 1) and not t["manifold"] and not t["closed"] and not t["oriented"]


def test_shape_record_and_figures():
    v, f = _soup([[(0, 0, 0), (1, 0, 0), (0.5, np.sqrt(3) / 2, 0)], [(0, 0, 0), (2, 0, 0), (1, 0, 0)], [(0, 0, 0), (3, 0, 0), (0, 4, 0)]])
    rec = QO.prepare(v, f, -1.0, 5.0)[2]
    alr, angle = QO.shape_figures(rec)
    assert abs(alr[0] - 1) < 1e-6 and alr[1] == 0 and abs(alr[2] - 12 * np.sqrt(3) * 6 / 144) < 1e-12
    assert abs(angle[0] - 60) < 1e-4 and angle[1] == 0 and abs(angle[2] - np.degrees(np.arctan2(3, 4))) < 1e-12


# ---------------------------------------------------------------- CPU: plumbing and argument checks ----------------------------------------------------------------
def test_build_lists_signatures_and_defaults():
    assert {"quality_kernels.hip", "quality_capi.cpp"} <= set(_build.SOURCES) and "quality.h" in _build.HEADERS
    assert _build.SOURCE_FLAGS["quality_kernels.hip"] == ["-ffp-contract=off"]
    for name in ("quality_kernels.hip", "quality_capi.cpp", "quality.h"):
        assert os.path.exists(os.path.join(_build.CSRC, name))
    names = {"tsamd_quality_info", "tsamd_quality_prepare", "tsamd_quality_pairs", "tsamd_quality_edges", "tsamd_quality_fan_pairs", "tsamd_quality_union"}
    assert names <= set(_capi.SIGNATURES)
    header = open(os.path.join(ROOT, "include", "tssplat_amd.h")).read()
    assert all(f" {n}(" in header for n in names)
    assert _capi.ABI_VERSION == 3 and _capi.load().tsamd_abi_version() == 3   # an addition is no incompatible change
    from tssplat_amd import geometry, quality
    assert {"self_intersections", "topology", "shape", "mesh_quality"} <= set(quality.__all__)
    sig = inspect.signature(quality.self_intersections).parameters
    assert (sig["bounds"].default, sig["max_pairs"].default) == (None, 65536) and sig["order"].default in quality.ORDERS and quality.ORDERS == ("none", "morton")
    assert "bounds" in inspect.signature(geometry.TetMeshGeometry.surface_quality).parameters
    info = quality.launch_info()
    assert info["block"] % 64 == 0 and info["tile"] % info["block"] == 0 and info["queue"] >= 128 and info["tile"] * 16 <= 64 * 1024


def test_c_abi_argument_errors_launch_nothing():
    """Every argument error is reported before anything touches the device: all device pointers here are null or made up."""
    lib = _capi.load()
    p, odd = 0x1000, 0x1002                                                 # "not null", aligned / not 4-byte aligned; never dereferenced on these paths

    def prepare(v=p, nv=3, f=p, nt=4, lo=0.0, hi=1.0, corners=p, boxes=p, state=p, shape=p, morton=p):
        return lib.tsamd_quality_prepare(v, nv, f, nt, lo, hi, corners, boxes, state, shape, morton, None)

    def pairs(corners=p, boxes=p, state=p, nt=4, tiles=None, cap=8, crossings=p, out=p, stats=p):
        return lib.tsamd_quality_pairs(corners, boxes, state, nt, tiles, cap, crossings, out, stats, None)

    def edges(f=p, state=p, nt=4, nv=3, und=p, dirk=p, vp=p, ref=p):
        return lib.tsamd_quality_edges(f, state, nt, nv, und, dirk, vp, ref, None)

    def fans(f=p, nt=4, keys=p, order=p, out=p):
        return lib.tsamd_quality_fan_pairs(f, nt, keys, order, out, None)

    def union(prs=p, npairs=4, labels=p, n=4, work=p):
        return lib.tsamd_quality_union(prs, npairs, labels, n, work, None, None)

    def info(out=(1, 1, 1)):
        slots = [C.c_int32() for _ in range(3)]
        return lib.tsamd_quality_info(*(C.byref(s) if keep else None for s, keep in zip(slots, out)))

    big = 2 ** 31
    cases = [
        (prepare, dict(nt=-1), "n_triangles"), (prepare, dict(nt=big // 3), "n_triangles"), (prepare, dict(nv=-1), "n_vertices"), (prepare, dict(nv=big), "n_vertices"),
        (prepare, dict(lo=1.0, hi=1.0), "lo must be below hi"), (prepare, dict(hi=float("nan")), "lo must be below hi"), (prepare, dict(hi=float("inf")), "lo must be below hi"),
        (prepare, dict(v=None), "v_dev"), (prepare, dict(f=None), "faces_dev"), (prepare, dict(corners=None), "corners_out_dev"), (prepare, dict(boxes=None), "boxes_out_dev"),
        (prepare, dict(state=None), "state_out_dev"), (prepare, dict(shape=None), "shape_out_dev"), (prepare, dict(morton=None), "morton_out_dev"),
        (prepare, dict(v=odd), "v_dev"), (prepare, dict(f=odd), "faces_dev"), (prepare, dict(corners=0x1004), "corners_out_dev"), (prepare, dict(shape=0x1004), "shape_out_dev"),
        (pairs, dict(nt=-1), "n_triangles"), (pairs, dict(cap=-1), "max_pairs"), (pairs, dict(cap=big), "max_pairs"), (pairs, dict(stats=None), "stats_out_dev"),
        (pairs, dict(corners=None), "corners_dev"), (pairs, dict(boxes=None), "boxes_dev"), (pairs, dict(state=None), "state_dev"),
        (pairs, dict(crossings=None), "crossings_out_dev"), (pairs, dict(out=None), "pairs_out_dev"), (pairs, dict(tiles=0x1004), "tile_boxes_dev"),
        (pairs, dict(stats=0x1004), "stats_out_dev"), (pairs, dict(crossings=odd), "crossings_out_dev"),
        (edges, dict(nt=-1), "n_triangles"), (edges, dict(nv=big), "n_vertices"), (edges, dict(f=None), "faces_dev"), (edges, dict(state=None), "state_dev"),
        (edges, dict(und=None), "und_keys_out_dev"), (edges, dict(dirk=0x1004), "dir_keys_out_dev"), (edges, dict(vp=None), "vertex_pairs_out_dev"),
        (edges, dict(ref=None), "referenced_out_dev"),
        (fans, dict(nt=-1), "n_triangles"), (fans, dict(f=None), "faces_dev"), (fans, dict(keys=None), "sorted_keys_dev"), (fans, dict(order=0x1004), "order_dev"),
        (fans, dict(out=None), "corner_pairs_out_dev"),
        (union, dict(n=-1), "n out"), (union, dict(n=big), "n out"), (union, dict(npairs=-1), "n_pairs"), (union, dict(labels=None), "labels_out_dev"),
        (union, dict(work=None), "workspace_dev"), (union, dict(prs=None), "pairs_dev"), (union, dict(labels=odd), "labels_out_dev"),
        (info, dict(out=(0, 1, 1)), "block_out"), (info, dict(out=(1, 0, 1)), "tile_out"), (info, dict(out=(1, 1, 0)), "queue_out"),
    ]
    for fn, kw, word in cases:
        assert fn(**kw) == INVALID, (fn.__name__, kw)
        msg = lib.tsamd_last_error().decode()
        assert msg and word in msg, (fn.__name__, kw, msg)
    # nothing to do is not an error, and still launches nothing
    assert prepare(nt=0, v=None, f=None, corners=None, boxes=None, state=None, shape=None, morton=None) == 0
    assert fans(nt=0, f=None, keys=None, order=None, out=None) == 0 and union(n=0, npairs=0, prs=None, labels=None, work=None) == 0
    assert pairs(cap=0, out=None, stats=None) == INVALID                    # (max_pairs = 0 takes no list; the stats are still needed)
    assert info() == 0 and _capi.ABI_VERSION == 3 and lib.tsamd_abi_version() == 3


def test_python_arguments_are_checked_by_name():
    """Nothing here reaches the library: a CPU tensor is refused first, with the argument's name."""
    from tssplat_amd import quality
    v, f = torch.zeros(4, 3), torch.zeros(1, 3, dtype=torch.int32)
    for call, word in [(lambda: quality.self_intersections(v, f), "v must be a GPU tensor"), (lambda: quality.self_intersections(v, f, max_pairs=-1), "max_pairs must be"),
                       (lambda: quality.self_intersections(v, f, max_pairs=1.5), "max_pairs must be"), (lambda: quality.self_intersections(v, f, order="hilbert"), "order must be"),
                       (lambda: quality.self_intersections(v, f, bounds=(1.0, 1.0)), "bounds must be"), (lambda: quality.self_intersections(v.double(), f), "v must be float32"),
                       (lambda: quality.self_intersections(v, f.long()), "faces must be int32"), (lambda: quality.topology(v, f), "v must be a GPU tensor"),
                       (lambda: quality.topology(v, f, bounds=(0.0,)), "bounds must be"), (lambda: quality.shape(None, f), "v must"),
                       (lambda: quality.mesh_quality(v, f, order=3), "order must be"), (lambda: quality.mesh_quality(v, f), "v must be a GPU tensor")]:
        with pytest.raises(RuntimeError, match="tssplat_amd.quality.*" + word):
            call()


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
    for want in ("quality_prepare_kernel", "quality_tile_boxes_kernel", "quality_pairs_kernel", "quality_finish_kernel", "quality_edges_kernel",
                 "quality_fan_pairs_kernel", "union_init_kernel", "union_hook_kernel", "union_compress_kernel"):
        recs = [v for k, v in meta.items() if want in k]
        assert len(recs) == 1, want
        assert recs[0]["vgpr_spill_count"] == 0 and recs[0]["private_segment_fixed_size"] == 0, (want, recs[0])


# ---------------------------------------------------------------- GPU: bytes ----------------------------------------------------------------
STATS = ("crossing_pairs", "crossing_faces", "invalid_faces", "degenerate_faces", "box_pairs")


def _assert_pairs(v, f, bounds, want, what, max_pairs=65536):
    """Both orders, each twice: crossings, sorted pairs and stats equal the oracle's bytes and each other's."""
    from tssplat_amd import quality
    dv, df = dev(v), dev(f)
    for order in quality.ORDERS:
        for run in range(2):
            got = quality.self_intersections(dv, df, bounds=bounds, max_pairs=max_pairs, order=order)
            assert got.crossings.dtype == torch.int32 and got.crossings.cpu().numpy().tobytes() == want["crossings"].tobytes(), (what, order, run)
            for key in STATS:
                assert getattr(got, key) == want[key], (what, order, run, key, getattr(got, key), want[key])
            assert got.pairs_truncated is False and got.pairs.dtype == torch.int64
            assert got.pairs.cpu().numpy().tobytes() == want["pairs"].tobytes(), (what, order, run)
            assert got.order == order and got.bounds == tuple(bounds)


@gpu
def test_hand_made_contacts_on_the_device():
    for name, second, expected in TABLE:
        v, f = _table_case(second)
        want = QO.self_intersections(v, f, *UNITY)
        assert want["crossing_pairs"] == expected
        _assert_pairs(v, f, UNITY, want, name)
    _assert_pairs(*_hostile(), UNITY, _pairs_oracle("hostile"), "hostile")
    # corners at the lattice extremes: the largest determinants
    v, f = _soup([[(0, 0, 0), (M, 0, M), (0, M, M)], [(M, M, 0), (0, M, 0), (3, 5, M)], [(0, 0, M), (M, M, M), (M, 0, 0)], [(0, M, 0), (M, 0, 0), (M, M, M)]])
    want = QO.self_intersections(v, f, *UNITY)
    assert want["crossing_pairs"] >= 1 and want["box_pairs"] == 6
    _assert_pairs(v, f, UNITY, want, "extremes")


@gpu
@pytest.mark.parametrize("which", ["block", "tile"])
def test_every_launch_edge_with_planted_crossings(which):
    """T around the workgroup's Q triangles and around the tile's K, with copies of one needle at 0, Q - 1, Q, K - 1, K and T - 1: pairs inside one
    block (the j > i rule on the diagonal), across a workgroup seam and across a tile seam."""
    from tssplat_amd import quality
    info = quality.launch_info()
    Q, K = info["block"], info["tile"]
    sizes = (1, 2, Q - 1, Q, Q + 1, 2 * Q + 1) if which == "block" else (K - 1, K, K + 1, 2 * K + 1)
    for T in sizes:
        for target in sorted({T // 2, min(T - 1, 3), min(T - 1, Q + 5)}):
            v, f, pairs = _planted(T, (0, Q - 1, Q, K - 1, K, T - 1), target)
            want = QO.self_intersections(v, f, *UNITY)
            assert want["pairs"].tolist() == pairs.tolist()
            _assert_pairs(v, f, UNITY, want, (T, target))


@gpu
@pytest.mark.parametrize("name,pairs", [("s1_sphere", 0), ("shifted_spheres", 272), ("mario", 18)])
def test_golden_meshes_equal_oracle(name, pairs):
    v, f, bounds = PAIR_MESHES[name]()
    want = _pairs_oracle(name)
    assert want["crossing_pairs"] == pairs                                  # the prototype's figure; the oracle is the authority
    _assert_pairs(v, f, bounds, want, name)


@gpu
def test_merged_and_simplified_surfaces_equal_oracle():
    from tssplat_amd import merge, quality, scenes, simplify
    bv, bt = scenes.kuhn_ball(2)
    bv = bv / np.linalg.norm(bv, axis=1).max()
    v = np.concatenate([bv * 0.4 + np.asarray([-0.2, 0.05, 0.0]), bv * 0.35 + np.asarray([0.25, -0.1, 0.1])]).astype(F32)
    e = np.concatenate([bt, bt + bv.shape[0]]).astype(np.int32)
    merged = merge.merge_tets(dev(v), dev(e), grid=17)
    small = simplify.simplify(merged.v, merged.faces, 6)
    for what, mesh in (("merged", merged), ("simplified", small)):
        mv, mf = mesh.v.cpu().numpy(), mesh.faces.cpu().numpy()
        bounds = _tight(mv)
        si, topo = QO.self_intersections(mv, mf, *bounds), QO.topology(mf, mv.shape[0])
        _assert_pairs(mv, mf, bounds, si, what)
        _assert_topology(mv, mf, bounds, topo, what)
        tight = bool(topo["closed"] and topo["manifold"] and topo["oriented"] and si["crossing_pairs"] == 0)
        assert quality.mesh_quality(mesh.v, mesh.faces, bounds=bounds).watertight is tight, what
        assert what != "merged" or (topo["closed"] and topo["oriented"] and topo["components"] == 1)     # what merge_tets promises for this scene


@gpu
def test_max_pairs_zero_exact_and_one_less():
    from tssplat_amd import quality
    v, f, bounds = PAIR_MESHES["mario"]()
    want = _pairs_oracle("mario")
    n = want["crossing_pairs"]
    dv, df = dev(v), dev(f)
    for order in quality.ORDERS:
        exact = quality.self_intersections(dv, df, bounds=bounds, max_pairs=n, order=order)
        assert exact.pairs_truncated is False and exact.pairs.cpu().numpy().tobytes() == want["pairs"].tobytes()
        for cap in (0, n - 1):
            got = quality.self_intersections(dv, df, bounds=bounds, max_pairs=cap, order=order)
            assert got.pairs is None and got.pairs_truncated is True and got.crossing_pairs == n
            assert got.crossings.cpu().numpy().tobytes() == want["crossings"].tobytes()
    v, f = _golden("s1_sphere")
    got = quality.self_intersections(dev(v), dev(f), max_pairs=0)             # nothing to list: not truncated
    assert got.pairs_truncated is False and got.pairs.numel() == 0 and got.crossing_pairs == 0


@gpu
def test_the_queue_drains_on_many_copies_of_one_pair():
    """200 copies of a triangle and of a needle through it: every wave's queue fills many times over."""
    from tssplat_amd import quality
    v, f, bounds = PAIR_MESHES["drain"]()
    want = _pairs_oracle("drain")
    assert want["crossing_pairs"] == 200 * 200 > 64 * quality.launch_info()["queue"] and want["box_pairs"] == 400 * 399 // 2
    _assert_pairs(v, f, bounds, want, "drain")


@gpu
def test_empty_and_all_invalid_meshes():
    from tssplat_amd import quality
    v, f = _golden("s1_sphere")
    for order in quality.ORDERS:
        got = quality.mesh_quality(dev(v), dev(f[:0]), order=order)
        assert got.intersections.crossing_pairs == 0 and got.intersections.crossings.numel() == 0 and got.intersections.pairs.numel() == 0
        assert got.topology.edges == 0 and got.topology.components == 0 and (got.topology.component == -1).all() and (got.topology.fans == 0).all()
        assert got.shape.faces == 0 and got.watertight is True              # vacuously
        bad = np.full_like(v, np.nan)
        for vv, ff, bounds in ((bad, f, (0.0, 1.0)), (v, f + v.shape[0], None), (v, f, (50.0, 60.0)), (v[:0], f, None)):
            got = quality.mesh_quality(dev(vv), dev(ff), bounds=bounds, order=order)
            si, topo = got.intersections, got.topology
            assert (si.invalid_faces, si.degenerate_faces, si.crossing_pairs, si.box_pairs) == (f.shape[0], 0, 0, 0) and int(si.crossings.abs().sum()) == 0
            assert (topo.edges, topo.components, topo.valid_faces, topo.euler) == (0, 0, 0, 0) and got.shape.faces == 0
            assert topo.component.numel() == vv.shape[0] and (topo.component == -1).all()


def _assert_topology(v, f, bounds, want, what):
    from tssplat_amd import quality
    for run in range(2):
        got = quality.topology(dev(v), dev(f), bounds=bounds)
        for key in ("edges", "boundary_edges", "nonmanifold_edges", "repeated_directed_edges", "oriented", "components", "nonmanifold_vertices", "manifold",
                    "euler", "closed", "valid_faces", "referenced_vertices"):
            assert getattr(got, key) == want[key] and type(getattr(got, key)) is type(want[key]), (what, run, key, getattr(got, key), want[key])
        assert got.component.dtype == torch.int32 and got.component.cpu().numpy().tobytes() == want["component"].tobytes(), (what, run)
        assert got.fans.dtype == torch.int32 and got.fans.cpu().numpy().tobytes() == want["fans"].tobytes(), (what, run)
    return got


@gpu
@pytest.mark.parametrize("name", sorted(TOPOLOGY_MESHES))
def test_topology_equals_oracle(name):
    from tssplat_amd import simplify
    v, f = TOPOLOGY_MESHES[name]()
    want, bounds = _topology_oracle(name)
    got = _assert_topology(v, f, bounds, want, name)
    if name not in ("hostile",):                                            # every face valid: edge_stats counts the same mesh
        assert tuple(simplify.edge_stats(dev(f))) == (got.edges, got.boundary_edges, got.nonmanifold_edges, got.closed)
    assert 1 <= got.union_rounds[1] <= 3 * f.shape[0] + 1


@gpu
def test_shape_record_bits_and_figures():
    from tssplat_amd import quality
    v, f = _golden("mario_mesh")
    bounds = _tight(v)
    rec = quality._prepare(dev(v), dev(f), *bounds)
    corners, state, shape = QO.prepare(v, f, *bounds)
    assert rec[3].cpu().numpy().tobytes() == shape.tobytes() and rec[2].cpu().numpy().tobytes() == state.tobytes()
    packed = corners[..., 0] | (corners[..., 1] << 21) | (corners[..., 2] << 42)
    good = state == QO.VALID
    assert (rec[0].cpu().numpy()[good] == packed[good]).all() and (rec[0].cpu().numpy()[~good] == -1).all()
    alr, angle = QO.shape_figures(shape)
    got = quality.shape(dev(v), dev(f))
    assert got.faces == alr.size
    for a, b in ((got.alr_mean, alr.mean()), (got.alr_min, alr.min()), (got.alr_p05, np.sort(alr)[int(np.floor(0.05 * (alr.size - 1)))]),
                 (got.alr_below_0p1, (alr < 0.1).mean()), (got.min_angle_min, angle.min()), (got.min_angle_mean, angle.mean())):
        assert abs(a - b) <= 1e-9 * max(1.0, abs(b)), (a, b)                # float64 sums in another order; sqrt and atan2 of two libraries
    assert 0 <= got.alr_min <= got.alr_p05 <= got.alr_mean <= 1 and 0 <= got.min_angle_min <= got.min_angle_mean <= 60 + 1e-9


@gpu
def test_mesh_quality_and_geometry_surface_quality():
    from tssplat_amd import geometry, quality, scenes
    v, f = _golden("s1_sphere")
    got = quality.mesh_quality(dev(v), dev(f))
    assert got.watertight is True and got.topology.euler == 2 and got.intersections.crossing_pairs == 0 and got.shape.faces == f.shape[0]
    v2, f2 = _shifted_spheres()
    got = quality.mesh_quality(dev(v2), dev(f2), bounds=_tight(v2))
    assert got.watertight is False and got.topology.closed and got.topology.manifold and got.intersections.crossing_pairs == 272
    assert dataclasses.asdict(dataclasses.replace(got.intersections, crossings=None, pairs=None))["crossing_faces"] == _pairs_oracle("shifted_spheres")["crossing_faces"]
    bv, bt = scenes.kuhn_ball(2)
    geo = geometry.TetMeshGeometry(bv.astype(F32), bt.astype(np.int32), use_smooth_barrier=False)
    sq = geo.surface_quality()
    assert isinstance(sq, quality.MeshQuality) and sq.watertight is True and sq.topology.components == 1 and sq.topology.euler == 2
