"""The surface simplifier (tssplat_amd/simplify.py: simplify, edge_stats; merge_tets(simplify=)): vertex clustering on a cube grid with
quadric placement.  It is separately rounded float64 operations, sequential sums and integers: the device results are compared
with tests/simplify_oracle.py bit for bit.  The oracle itself is checked on the CPU: containment in the cells, a plane that must
stay a plane, the fallbacks of the solve, quadric against mean placement through the surface metrics' oracle."""
import dataclasses
import functools
import inspect
import os
import sys

import numpy as np
import pytest
import torch

import metrics_oracle as MO
import simplify_oracle as SO
from tssplat_amd import _build, _capi, scenes

gpu = pytest.mark.gpu
INVALID = 1     # TSAMD_ERR_INVALID_ARGUMENT
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
UNIT = (-1.0, 1.0)
COUNTS = ("cells_occupied", "clamped", "duplicates", "degenerate_faces", "invalid_faces")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------- meshes ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden(name):
    d = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    return np.ascontiguousarray(d["vertices"], dtype=F32), np.ascontiguousarray(d["faces"], dtype=np.int32)


def _one_triangle():
    return np.array([[0.25, -1, 3], [2, 0.5, 3.5], [-1, 1.5, 2]], F32), np.array([[0, 1, 2]], np.int32)


def _tetrahedron():
    v = np.array([[-0.5, -0.4, -0.45], [0.6, -0.3, -0.5], [-0.2, 0.7, -0.35], [0.1, 0.05, 0.65]], F32)
    return v, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.int32)


def _hostile_mesh():
    """Face 0: fine.  1: a repeated corner.  2: a NaN vertex.  3: an index past the end.  4: a negative index.  5: a sliver of 2^-17 legs.
    6: collinear corners.  7: fine.  8: an infinite vertex."""
    s = 2.0 ** -17
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [5, 5, 5], [5 + s, 5, 5], [5, 5 + s, 5], [2, 2, 2], [3, 3, 3], [4, 4, 4],
                  [0, 0, 1], [0.5, 0, 1], [0, 0.5, 1], [np.inf, 0, 0]], F32)
    f = np.array([[0, 1, 2], [0, 1, 1], [0, 3, 2], [0, 1, 14], [0, -1, 2], [4, 5, 6], [7, 8, 9], [10, 11, 12], [0, 13, 2]], np.int32)
    return v, f


def _plane():
    """A 9 x 9 grid of vertices at z = 0.3 over [0, 1]^2, 128 triangles: vertices on the faces between the cells of C = 4 and on `hi`."""
    x = np.arange(9) / 8.0
    X, Y = np.meshgrid(x, x, indexing="ij")
    v = np.stack([X, Y, np.full_like(X, 0.3)], -1).reshape(-1, 3).astype(F32)
    idx = np.arange(81).reshape(9, 9)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    return v, np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.int32)


def _collinear():
    """One triangle with collinear corners in three cells of C = 4 on [0, 1]: n = 0, so tr = 0 and the placement is the mean."""
    return np.array([[0.1, 0.1, 0.1], [0.4, 0.4, 0.4], [0.9, 0.9, 0.9]], F32), np.array([[0, 1, 2]], np.int32)


def _fan():
    """300 triangles around one centre vertex with a ring of 300 vertices far away: at C = 8 on [-1, 1] the centre's cell has a run of 300
    records next to the ring cells' short ones."""
    n = 300
    ang = 2 * np.pi * np.arange(n) / n
    ring = np.stack([0.85 * np.cos(ang), 0.85 * np.sin(ang), 0.1 + 0.3 * np.sin(3 * ang)], 1)
    v = np.concatenate([[[0.1, 0.12, 0.07]], ring]).astype(F32)
    i = np.arange(n)
    return v, np.stack([np.zeros(n, np.int64), 1 + i, 1 + (i + 1) % n], 1).astype(np.int32)


def _two_spheres():
    """tests/test_merge.py's overlapping two-sphere scene."""
    bv, bt = scenes.kuhn_ball(2)
    bv = bv / np.linalg.norm(bv, axis=1).max()
    v = np.concatenate([bv * 0.4 + np.asarray([-0.2, 0.05, 0.0]), bv * 0.35 + np.asarray([0.25, -0.1, 0.1])]).astype(F32)
    return v, np.concatenate([bt, bt + bv.shape[0]]).astype(np.int32)


MESHES = {"s1_sphere": lambda: _golden("s1_sphere"), "mario": lambda: _golden("mario_mesh"), "hostile": _hostile_mesh, "one_triangle": _one_triangle,
          "tetrahedron": _tetrahedron, "plane": _plane, "collinear": _collinear, "fan": _fan}


# ---- the launch edges ----
TOP_KEY = 1024 ** 3 - 1                            # the last cell of the finest grid: 2^30 - 1


def _corner_mesh():
    """On the bounds (0, 1): vertices exactly on lo and exactly on hi on all three axes (cell 0, and the last cell through the clamp),
    on one or two axes, and on interior cell faces of C = 1024 (0.5 = 512 h, 0.25 = 256 h, 0.75 = 768 h)."""
    v = np.array([[0, 0, 0], [1, 1, 1], [1, 0, 0], [0, 1, 0], [0.5, 0.5, 0.5], [0.25, 0.75, 0.5], [1, 1, 0], [0, 0, 1], [0.75, 1, 0.25], [1, 0.5, 1]], F32)
    f = np.array([[0, 2, 3], [1, 3, 2], [0, 4, 1], [4, 5, 1], [2, 6, 1], [7, 0, 4], [8, 1, 5], [9, 1, 4], [6, 8, 1], [7, 4, 9]], np.int32)
    return v, f


def _first_triangles(n):
    v, f = _golden("s1_sphere")
    return v, np.ascontiguousarray(f[:n])


def _first_vertices(n):
    """The golden sphere's first n vertices and the faces among them."""
    v, f = _golden("s1_sphere")
    return np.ascontiguousarray(v[:n]), np.ascontiguousarray(f[(f < n).all(axis=1)])


DEDUPE_CELLS = 8


def _sorted_survivors(v, f, cells, bounds=None):
    """The input indices of the faces with three distinct cells, in the order of (rotated cell triple, input index): the order the
    dedupe walks.  From the oracle's vertex keys alone."""
    keys = SO.simplify(v, f, cells, bounds)["vertex_keys"][f]
    assert (keys >= 0).all()
    idx = np.nonzero((keys[:, 0] != keys[:, 1]) & (keys[:, 0] != keys[:, 2]) & (keys[:, 1] != keys[:, 2]))[0]
    rot = np.stack([np.roll(row, -int(row.argmin())) for row in keys[idx]])
    return idx[np.lexsort((idx, rot[:, 2], rot[:, 1], rot[:, 0]))], idx


def _dedupe_boundary_mesh():
    """The golden sphere with the survivor at sorted position 255 moved to input index 255 and a rotated copy of it inserted at input
    index 256: the pair sits at input indices 255 | 256 and at sorted positions 255 | 256, either side of a workgroup."""
    v, f = _golden("s1_sphere")
    order, _ = _sorted_survivors(v, f, DEDUPE_CELLS)
    f = f.copy()
    x = int(order[255])
    f[[255, x]] = f[[x, 255]]
    return v, np.ascontiguousarray(np.insert(f, 256, f[255][[1, 2, 0]], axis=0))


MESHES.update({"corners": _corner_mesh, "tri256": lambda: _first_triangles(256), "tri257": lambda: _first_triangles(257), "vert256": lambda: _first_vertices(256),
               "vert257": lambda: _first_vertices(257), "dedupe_boundary": _dedupe_boundary_mesh})


@functools.lru_cache(maxsize=None)
def _oracle(mesh, cells, bounds=None, placement="quadric"):
    return SO.simplify(*MESHES[mesh](), cells, bounds, placement)


def _np_edge_stats(faces):
    """A restatement with a dictionary of directed edges, independent of the oracle's sorted keys."""
    und, seen_twice = {}, False
    directed = set()
    for t in np.asarray(faces).reshape(-1, 3).tolist():
        for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            und[(min(a, b), max(a, b))] = und.get((min(a, b), max(a, b)), 0) + 1
            seen_twice = seen_twice or (a, b) in directed
            directed.add((a, b))
    counts = np.array(list(und.values()), np.int64)
    return len(und), int((counts == 1).sum()), int((counts > 2).sum()), bool((counts == 2).all() and not seen_twice)


# ---------------------------------------------------------------- CPU: the oracle ----------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["s1_sphere", "mario"])
@pytest.mark.parametrize("cells", [4, 16, 32])
def test_oracle_containment(mesh, cells):
    """Every output vertex lies in its cell's closed box [g - h/2, g + h/2]: the position is a float64 in that box rounded once to float32,
    and rounding is monotone, so the float32 lies between the float32 roundings of the box's ends.  Hence every valid input vertex is
    within sqrt(3) h, the box's diagonal, of its cell's representative."""
    v, f = MESHES[mesh]()
    for placement in SO.PLACEMENTS:
        r = _oracle(mesh, cells, None, placement)
        lo, hi = r["bounds"]
        box_lo, box_hi = SO.cell_boxes(r["keys"], cells, lo, hi)
        assert r["v"].shape[0] == r["keys"].shape[0] > 0
        assert (r["v"] >= box_lo.astype(F32)).all() and (r["v"] <= box_hi.astype(F32)).all()
        # every occupied cell's representative, used by a surviving face or not
        all_lo, all_hi = SO.cell_boxes(r["cell_keys"], cells, lo, hi)
        assert (r["cell_pos"] >= all_lo.astype(F32)).all() and (r["cell_pos"] <= all_hi.astype(F32)).all()
        referenced = np.unique(f)                                       # vertices of a valid face have a record, so their cell is occupied
        rep = r["cell_pos"][np.searchsorted(r["cell_keys"], r["vertex_keys"][referenced])].astype(np.float64)
        dist = np.linalg.norm(v[referenced].astype(np.float64) - rep, axis=1)
        print(f"{mesh} C={cells} {placement}: max distance {dist.max():.4f} bound {np.sqrt(3.0) * r['h']:.4f}")
        assert (dist <= np.sqrt(3.0) * r["h"]).all()
        assert r["faces"].min() == 0 and r["faces"].max() == r["v"].shape[0] - 1 and np.unique(r["faces"]).shape[0] == r["v"].shape[0]   # no vertex unreferenced
        assert (np.diff(r["keys"]) > 0).all()


def test_oracle_plane_stays_a_plane():
    """z = 0.3 everywhere: the final rounding to float32 is 2^-24 relative and the float64 noise far below it."""
    v, f = _plane()
    for placement in SO.PLACEMENTS:
        r = SO.simplify(v, f, 4, (0.0, 1.0), placement)
        err = np.abs(r["v"][:, 2].astype(np.float64) - np.float64(F32(0.3))).max()
        print(f"{placement}: vertices {r['v'].shape[0]} triangles {r['faces'].shape[0]} max |z - 0.3| {err:.3e}")
        assert r["v"].shape[0] == 16 and r["faces"].shape[0] == 18 and err <= 2.0 ** -22     # 4 x 4 cells of the plane, 3 x 3 x 2 triangles
        assert r["cells_occupied"] == 16 and r["invalid_faces"] == 0 and r["degenerate_faces"] == 128 - 18
    # the index clamp: x = 1.0 = hi belongs to the last cell, and a vertex outside the bounds to the border cell
    keys, _ = SO.vertex_keys(np.array([[1.0, 0.0, 0.25], [7.0, -3.0, 0.2499]], F32), 4, 0.0, 1.0)
    assert keys.tolist() == [(3 * 4 + 0) * 4 + 1, (3 * 4 + 0) * 4 + 0]


def test_oracle_fallbacks_and_invalid_faces():
    v, f = _collinear()
    q, m = SO.simplify(v, f, 4, (0.0, 1.0), "quadric"), SO.simplify(v, f, 4, (0.0, 1.0), "mean")
    assert q["v"].tobytes() == m["v"].tobytes() == v.tobytes() and q["faces"].tolist() == [[0, 1, 2]]      # tr = 0: the mean of one vertex is that vertex
    v, f = _hostile_mesh()
    r = SO.simplify(v, f, 8)
    assert r["bounds"] == (0.0, float(F32(5 + 2.0 ** -17)))
    # h = 0.625.  Invalid: faces 2, 3, 4, 8.  One cell: the repeated corner (1), the sliver (5) and face 7, whose legs of 0.5 stay in cell 0 of
    # x and y.  Three cells: face 0 and the collinear face 6
    assert r["invalid_faces"] == 4 and r["degenerate_faces"] == 3
    assert r["faces"].shape[0] == 2 and r["duplicates"] == 0 and np.isfinite(r["v"]).all()
    assert (r["vertex_keys"][[3, 13]] == -1).all() and (np.delete(r["vertex_keys"], [3, 13]) >= 0).all()
    poisoned = v.copy()
    poisoned[[3, 13]] = 1e30                                              # what an access through faces 2 and 8 would have read
    again = SO.simplify(v, f, 8, r["bounds"])
    assert again["v"].tobytes() == r["v"].tobytes()
    assert SO.simplify(poisoned, f[[0, 1, 5, 6, 7]], 8, r["bounds"])["v"].tobytes() == r["v"].tobytes()
    for vv, bounds in ((np.full((3, 3), np.nan, F32), None), (np.ones((3, 3), F32), None), (v, (1.0, 1.0)), (v, (0.0, np.inf))):
        with pytest.raises(RuntimeError, match="simplify"):
            SO.simplify(vv, f[:1], 4, bounds)


def test_oracle_quadric_beats_mean_on_the_sphere():
    """The accuracy (mean distance from samples of the output to samples of the input) of the two placements on s1_sphere at C = 4, through
    tests/metrics_oracle.py.  Mean placement pulls every vertex inside the sphere; the quadric's minimum lies near the surface."""
    v, f = _golden("s1_sphere")
    n = 2000
    ref = MO.sample_surface(v, f, n, 0)
    acc = {}
    for placement in SO.PLACEMENTS:
        r = _oracle("s1_sphere", 4, None, placement)
        acc[placement] = MO.compare(MO.sample_surface(r["v"], r["faces"], n, 2), ref)["accuracy"]
    print(f"accuracy quadric {acc['quadric']:.4f} mean {acc['mean']:.4f} at {n} samples")
    assert acc["quadric"] < acc["mean"]


def test_oracle_other_cases_and_edge_stats():
    for mesh in ("s1_sphere", "mario", "one_triangle"):
        r = _oracle(mesh, 1)
        assert r["v"].shape == (0, 3) and r["faces"].shape == (0, 3) and r["cells_occupied"] == 1 and r["degenerate_faces"] == MESHES[mesh]()[1].shape[0]
    assert _oracle("mario", 2)["duplicates"] > 0
    assert _oracle("s1_sphere", 1)["run_lengths"].tolist() == [2996]
    t = _oracle("tetrahedron", 2, UNIT)
    assert t["v"].shape == (4, 3) and t["faces"].shape == (4, 3) and SO.edge_stats(t["faces"]) == (6, 0, 0, True)
    # orientation: a rotation keeps it, so the surviving tetrahedron's signed volume keeps its sign
    vol = lambda vv, ff: sum(np.dot(vv[a].astype(np.float64), np.cross(vv[b].astype(np.float64), vv[c].astype(np.float64))) for a, b, c in ff.tolist())
    assert vol(*_tetrahedron()) * vol(t["v"], t["faces"]) > 0
    for faces in (_oracle("s1_sphere", 8)["faces"], _oracle("s1_sphere", 16)["faces"], _oracle("mario", 32)["faces"], _golden("mario_mesh")[1], _plane()[1],
                  np.array([[0, 1, 2], [0, 1, 2]]), np.array([[0, 1, 2], [2, 1, 0]]), np.zeros((0, 3), np.int32)):
        assert SO.edge_stats(faces) == _np_edge_stats(faces)
    assert SO.edge_stats(_oracle("s1_sphere", 16)["faces"])[3] and SO.edge_stats(_oracle("s1_sphere", 8)["faces"])[2] == 2      # closed is reported, never promised
    assert SO.edge_stats(_plane()[1]) == (208, 32, 0, False) and SO.edge_stats(np.array([[0, 1, 2], [0, 1, 2]])) == (3, 0, 0, False)
    # opposite-orientation twins are kept, equal triples are not
    v = np.array([[0.1, 0.1, 0.1], [0.9, 0.1, 0.1], [0.1, 0.9, 0.1], [0.15, 0.12, 0.1]], F32)
    r = SO.simplify(v, np.array([[0, 1, 2], [2, 1, 0], [1, 2, 3], [3, 1, 2]], np.int32), 2, (0.0, 1.0))
    assert r["faces"].tolist() == [[0, 2, 1], [0, 1, 2]] and r["duplicates"] == 2


# ---------------------------------------------------------------- CPU: the launch edges are reached ----------------------------------------------------------------
FINE_CELLS = [1023, 1024]
BLOCK_MESHES = ["tri256", "tri257", "vert256", "vert257"]
BLOCK_CELLS = 64
UNIT01 = (0.0, 1.0)


def _fine_preconditions(mesh, cells):
    """Keys need 30 bits: the decode in the run walk and every 32-bit product on the way are exercised."""
    r = _oracle(mesh, cells)
    assert r["cell_keys"].max() >= 2 ** 29 and r["faces"].shape[0] > 0.9 * MESHES[mesh]()[1].shape[0]
    return r


@pytest.mark.parametrize("cells", FINE_CELLS)
@pytest.mark.parametrize("mesh", ["s1_sphere", "mario"])
def test_edge_finest_grids_are_reached(mesh, cells):
    _fine_preconditions(mesh, cells)


def _corner_preconditions(cells, placement="quadric"):
    r = _oracle("corners", cells, UNIT01, placement)
    top = cells ** 3 - 1
    v, f = _corner_mesh()
    assert r["vertex_keys"][0] == 0 and r["vertex_keys"][1] == top == r["cell_keys"].max() == r["keys"].max() and r["keys"].min() == 0
    assert (r["faces"] == r["v"].shape[0] - 1).any(axis=1).sum() >= 3                        # faces that survive with the last cell as a corner
    assert r["invalid_faces"] == 0 and r["degenerate_faces"] == 0 and r["faces"].shape[0] == f.shape[0]
    if cells == 1024:
        assert top == TOP_KEY == 2 ** 30 - 1
        on_face = (v * 1024 == np.floor(v * 1024)).all(axis=1) & ((v > 0) & (v < 1)).all(axis=1)
        assert on_face.sum() >= 2                                                             # vertices on interior cell faces
    return r


@pytest.mark.parametrize("cells", FINE_CELLS + [4])
def test_edge_corner_cells_are_reached(cells):
    for placement in SO.PLACEMENTS:
        r = _corner_preconditions(cells, placement)
        print(f"corners C={cells} {placement}: clamped {r['clamped']} of {r['cells_occupied']} cells")
    assert cells != 1023 or _corner_preconditions(cells, "quadric")["clamped"] > 0           # at 1023 the count is not trivially 0


def _block_preconditions(mesh):
    v, f = MESHES[mesh]()
    r = _oracle(mesh, BLOCK_CELLS)
    assert r["faces"].shape[0] > 0 and r["invalid_faces"] == 0
    if mesh.startswith("tri"):
        assert f.shape[0] == int(mesh[-3:]) and len(set(r["vertex_keys"][f[-1]].tolist())) == 3      # the last face has three cells: it survives
    else:
        assert v.shape[0] == int(mesh[-3:]) and (f == v.shape[0] - 1).any() and r["vertex_keys"][-1] in r["keys"]     # the last vertex's cell is in the output


@pytest.mark.parametrize("mesh", BLOCK_MESHES)
def test_edge_block_sized_meshes_are_reached(mesh):
    """256: the last lane of a workgroup is the last item.  257: a workgroup of one lane."""
    _block_preconditions(mesh)


def test_edge_dedupe_across_a_workgroup_is_reached():
    v, f = _dedupe_boundary_mesh()
    assert f.shape[0] == 2997 and f[256].tolist() == f[255][[1, 2, 0]].tolist()
    order, survivors = _sorted_survivors(v, f, DEDUPE_CELLS)
    assert order[255] == 255 and order[256] == 256                                           # sorted positions 255 | 256: order[p - 1] is another workgroup's
    before = _oracle("s1_sphere", DEDUPE_CELLS)
    r = _oracle("dedupe_boundary", DEDUPE_CELLS)
    assert r["duplicates"] == before["duplicates"] + 1 and r["faces"].shape[0] == before["faces"].shape[0]


# ---------------------------------------------------------------- CPU: plumbing and argument checks ----------------------------------------------------------------
def test_build_lists_signatures_and_defaults():
    assert {"simplify_kernels.hip", "simplify_capi.cpp"} <= set(_build.SOURCES) and "simplify.h" in _build.HEADERS
    assert _build.SOURCE_FLAGS["simplify_kernels.hip"] == ["-ffp-contract=off"]
    for name in ("simplify_kernels.hip", "simplify_capi.cpp", "simplify.h"):
        assert os.path.exists(os.path.join(_build.CSRC, name))
    assert {"tsamd_simplify_keys", "tsamd_simplify_cells", "tsamd_simplify_faces", "tsamd_simplify_dedupe"} <= set(_capi.SIGNATURES)
    assert _capi.ABI_VERSION == 3 and _capi.load().tsamd_abi_version() == 3
    from tssplat_amd import geometry, merge, renderers, simplify
    assert inspect.signature(simplify.simplify).parameters["placement"].default == "quadric"
    assert inspect.signature(simplify.simplify).parameters["stabilise"].default == 2.0 ** -10 == SO.DEFAULT_STABILISE
    for fn in (merge.merge_tets, geometry.TetMeshGeometry.export_merged, renderers.MeshRasterizer.export_merged):
        assert inspect.signature(fn).parameters["simplify"].default is None
    assert [f.name for f in dataclasses.fields(merge.MergedSurface)][-1] == "simplified"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import train_object
    finally:
        sys.path.pop(0)
    assert inspect.signature(train_object.run).parameters["merge_simplify"].default == 0
    assert '"--merge-simplify", type=int, default=0' in inspect.getsource(train_object.main)


def test_c_abi_argument_errors_launch_nothing():
    """Every argument error is reported before anything touches the device: all device pointers here are null or made up."""
    lib = _capi.load()
    p, odd, half = 0x1000, 0x1002, 0x1004

    def keys(v=p, nv=3, f=p, nt=1, cells=4, lo=0.0, hi=1.0, vkey=p, rec=p, state=p):
        return lib.tsamd_simplify_keys(v, nv, f, nt, cells, lo, hi, vkey, rec, state, None)

    def cells_(v=p, nv=3, f=p, nt=1, cells=4, lo=0.0, hi=1.0, placement=0, stab=0.0, vkey=p, rec=p, perm=p, pos=p, head=p, run=p, status=p):
        return lib.tsamd_simplify_cells(v, nv, f, nt, cells, lo, hi, placement, stab, vkey, rec, perm, pos, head, run, status, None)

    def faces(run=p, state=p, nt=1, tri=p, ab=p, c=p):
        return lib.tsamd_simplify_faces(run, state, nt, tri, ab, c, None)

    def dedupe(tri=p, order=p, nt=1, keep=p, used=p, status=p):
        return lib.tsamd_simplify_dedupe(tri, order, nt, keep, used, status, None)

    big = 2 ** 31
    cases = [
        (keys, dict(nv=-1), "n_vertices"), (keys, dict(nv=big), "n_vertices"), (keys, dict(nt=-1), "n_triangles"), (keys, dict(nt=(big - 1) // 3 + 1), "n_triangles"),
        (keys, dict(cells=0), "cells"), (keys, dict(cells=1025), "cells"), (keys, dict(lo=1.0), "lo / hi"), (keys, dict(hi=float("nan")), "lo / hi"),
        (keys, dict(hi=float("inf")), "lo / hi"), (keys, dict(lo=0.0, hi=5e-324), "lo / hi"), (keys, dict(v=None), "v_dev"), (keys, dict(f=None), "faces_dev"),
        (keys, dict(vkey=None), "vkey_out_dev"), (keys, dict(rec=None), "records_out_dev"), (keys, dict(state=None), "state_out_dev"), (keys, dict(v=odd), "v_dev"),
        (keys, dict(rec=half), "records_out_dev"),
        (cells_, dict(placement=2), "placement"), (cells_, dict(stab=-1.0), "stabilise"), (cells_, dict(stab=float("nan")), "stabilise"), (cells_, dict(cells=0), "cells"),
        (cells_, dict(nt=-1), "n_triangles"), (cells_, dict(status=None), "status_out_dev"), (cells_, dict(vkey=None), "vkey_dev"), (cells_, dict(rec=None), "records_dev"),
        (cells_, dict(perm=None), "perm_dev"), (cells_, dict(pos=None), "pos_out_dev"), (cells_, dict(head=None), "head_out_dev"), (cells_, dict(run=None), "run_out_dev"),
        (cells_, dict(perm=half), "perm_dev"), (cells_, dict(run=odd), "run_out_dev"),
        (faces, dict(nt=-1), "n_triangles"), (faces, dict(run=None), "run_dev"), (faces, dict(state=None), "state_dev"), (faces, dict(tri=None), "tri_out_dev"),
        (faces, dict(ab=None), "key_ab_out_dev"), (faces, dict(c=None), "key_c_out_dev"), (faces, dict(ab=half), "key_ab_out_dev"),
        (dedupe, dict(nt=-1), "n_triangles"), (dedupe, dict(tri=None), "tri_dev"), (dedupe, dict(order=None), "order_dev"), (dedupe, dict(keep=None), "keep_out_dev"),
        (dedupe, dict(used=None), "used_out_dev"), (dedupe, dict(status=None), "status_out_dev"), (dedupe, dict(order=half), "order_dev"),
    ]
    for fn, kw, word in cases:
        assert fn(**kw) == INVALID, (fn.__name__, kw)
        msg = lib.tsamd_last_error().decode()
        assert msg and word in msg, (fn.__name__, kw, msg)
    assert faces(nt=0, run=None, state=None, tri=None, ab=None, c=None) == 0       # nothing to do is not an error, and launches nothing
    assert _capi.ABI_VERSION == 3 and lib.tsamd_abi_version() == 3


def test_python_arguments_are_checked_by_name():
    """Nothing here reaches the library: wrong cells, bounds, placement, dtype, shape or device are refused first, by name."""
    from tssplat_amd import merge, simplify
    v, f = torch.zeros(4, 3), torch.zeros(1, 3, dtype=torch.int32)
    S = simplify.simplify
    for call, word in [(lambda: S(v, f, 0), "cells must be an integer in 1 .. 1024"), (lambda: S(v, f, 1025), "cells must"), (lambda: S(v, f, 2.0), "cells must"),
                       (lambda: S(v, f, True), "cells must"), (lambda: S(v, f, 4, placement="median"), "placement must be one of 'quadric', 'mean'"),
                       (lambda: S(v, f, 4, placement=None), "placement must"), (lambda: S(v, f, 4, stabilise=-1.0), "stabilise must"),
                       (lambda: S(v, f, 4, stabilise=float("nan")), "stabilise must"), (lambda: S(v, f, 4, bounds=(1.0, 1.0)), r"bounds must be \(lo, hi\)"),
                       (lambda: S(v, f, 4, bounds=(0.0, 1.0, 2.0)), "bounds must"), (lambda: S(v, f, 4, bounds=(0.0, float("inf"))), "bounds must"),
                       (lambda: S(v, f, 4, bounds=3), "bounds must"), (lambda: S(v.double(), f, 4), "v must be float32, got float64"),
                       (lambda: S(v, f.long(), 4), "faces must be int32, got int64"), (lambda: S(v[:, :2], f, 4), r"v must be \[N, 3\]"),
                       (lambda: S(v, f.reshape(-1), 4), r"faces must be \[N, 3\]"), (lambda: S(np.zeros((4, 3), F32), f, 4), "v must be a GPU tensor"),
                       (lambda: S(v, f, 4), "v must be a GPU tensor"), (lambda: S(v, f, 4, bounds=UNIT), "v must be a GPU tensor"),
                       (lambda: simplify.edge_stats(f.long()), "faces must be int32"), (lambda: simplify.edge_stats(f), "faces must be a GPU tensor"),
                       (lambda: simplify.run_lengths(v, f, 0), "cells must"),
                       (lambda: merge._check_simplify("merge_tets", 1, 32), "simplify must be None or an integer in 2 .. grid = 32"),
                       (lambda: merge._check_simplify("merge_tets", 33, 32), "simplify must"), (lambda: merge._check_simplify("merge_tets", 2.0, 32), "simplify must"),
                       (lambda: merge._check_simplify("merge_tets", True, 32), "simplify must")]:
        with pytest.raises(RuntimeError, match=word):
            call()
    assert merge._check_simplify("merge_tets", None, 32) is None and merge._check_simplify("merge_tets", 32, 32) == 32
    with pytest.raises(RuntimeError, match="status 1"):
        simplify._check_status("simplify", 1)


# ---------------------------------------------------------------- GPU: bit for bit against the oracle ----------------------------------------------------------------
def _assert_equal(got, want, what):
    assert got.v.dtype == torch.float32 and got.faces.dtype == torch.int32 and got.v.dim() == got.faces.dim() == 2
    gv, gf = got.v.cpu().numpy(), got.faces.cpu().numpy()
    assert gf.shape == want["faces"].shape and gv.shape == want["v"].shape, (what, gv.shape, gf.shape, want["v"].shape, want["faces"].shape)
    assert gf.tobytes() == want["faces"].tobytes(), (what, int((gf != want["faces"]).sum()))
    assert gv.tobytes() == want["v"].tobytes(), (what, int((gv.view(np.uint32) != want["v"].view(np.uint32)).sum()))
    for key in COUNTS:
        assert getattr(got, key) == want[key], (what, key, getattr(got, key), want[key])
    assert (got.cells, got.bounds, got.placement) == (want["cells"], want["bounds"], want["placement"])


def _both(mesh, cells, bounds=None, placements=SO.PLACEMENTS):
    from tssplat_amd import simplify
    v, f = (dev(x) for x in MESHES[mesh]())
    out = None
    for placement in placements:
        out = simplify.simplify(v, f, cells, bounds=bounds, placement=placement)
        _assert_equal(out, _oracle(mesh, cells, bounds, placement), (mesh, cells, bounds, placement))
    return out


@gpu
def test_small_meshes_equal_oracle():
    assert tuple(_both("one_triangle", 1).v.shape) == (0, 3)
    assert tuple(_both("one_triangle", 5).faces.shape) == (1, 3)
    assert tuple(_both("tetrahedron", 2, UNIT).faces.shape) == (4, 3)
    got = _both("hostile", 8)
    assert got.invalid_faces == 4 and got.degenerate_faces == 3 and tuple(got.faces.shape) == (2, 3)
    _both("hostile", 3, (0.5, 4.5))
    assert tuple(_both("plane", 4, (0.0, 1.0)).v.shape) == (16, 3)
    from tssplat_amd import simplify
    v, f = (dev(x) for x in _collinear())
    q, m = _both("collinear", 4, (0.0, 1.0), ("quadric",)), _both("collinear", 4, (0.0, 1.0), ("mean",))
    assert torch.equal(q.v, m.v) and torch.equal(q.v, v)
    empty = simplify.simplify(v, f[:0], 4, bounds=(0.0, 1.0))                # no face at all
    assert tuple(empty.v.shape) == (0, 3) and tuple(empty.faces.shape) == (0, 3) and empty.cells_occupied == 0
    none = simplify.simplify(v[:0], f, 4, bounds=(0.0, 1.0))                # no vertex: every face is invalid
    assert tuple(none.faces.shape) == (0, 3) and none.invalid_faces == 1
    for call, word in [(lambda: simplify.simplify(v[:0], f, 4), "no finite coordinate"), (lambda: simplify.simplify(v[:1], f, 4), "spans no interval"),
                       (lambda: simplify.simplify(v, f.cpu(), 4), "faces must be a GPU tensor")]:
        with pytest.raises(RuntimeError, match=word):
            call()


@gpu
@pytest.mark.parametrize("cells", [1, 2, 8, 16])
def test_sphere_equals_oracle(cells):
    """C = 1: a single run of 2 996 records, longer than any workgroup."""
    _both("s1_sphere", cells)


@gpu
@pytest.mark.parametrize("cells", [2, 32])
def test_mario_equals_oracle(cells):
    got = _both("mario", cells)
    assert got.duplicates > 0


@gpu
def test_fan_and_clamped_bounds_equal_oracle():
    from tssplat_amd import simplify
    got = _both("fan", 8, UNIT)
    assert tuple(got.faces.shape)[0] > 0
    lengths = simplify.run_lengths(dev(_fan()[0]), dev(_fan()[1]), 8, UNIT).cpu().numpy()
    assert lengths.tolist() == _oracle("fan", 8, UNIT)["run_lengths"].tolist() and lengths.max() == 300 and np.median(lengths) < 30
    _both("fan", 8)                                                       # bounds=None: the min / max of the coordinates
    _both("s1_sphere", 6, (-0.5, 0.7))                                    # part of the mesh outside: clamped keys
    _both("mario", 7, (0.0, 0.25))


@gpu
def test_runs_repeat_bit_for_bit_on_any_stream():
    from tssplat_amd import simplify
    v, f = (dev(x) for x in _golden("mario_mesh"))
    a, b = simplify.simplify(v, f, 32), simplify.simplify(v, f, 32)
    assert torch.equal(a.v.view(torch.int32), b.v.view(torch.int32)) and torch.equal(a.faces, b.faces)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = simplify.simplify(v, f, 32)
    side.synchronize()
    assert torch.equal(a.v.view(torch.int32), c.v.view(torch.int32)) and torch.equal(a.faces, c.faces)
    for other in (b, c):
        assert dataclasses.asdict(dataclasses.replace(a, v=None, faces=None)) == dataclasses.asdict(dataclasses.replace(other, v=None, faces=None))


@gpu
def test_edge_stats_equals_numpy():
    from tssplat_amd import simplify
    for mesh, cells in (("s1_sphere", 2), ("s1_sphere", 8), ("s1_sphere", 16), ("mario", 32)):
        got = simplify.simplify(*(dev(x) for x in MESHES[mesh]()), cells)
        stats = simplify.edge_stats(got.faces)
        assert tuple(stats) == _np_edge_stats(_oracle(mesh, cells)["faces"]), (mesh, cells)
    assert simplify.edge_stats(dev(_oracle("s1_sphere", 8)["faces"])).nonmanifold_edges == 2 and not simplify.edge_stats(dev(_oracle("s1_sphere", 8)["faces"])).closed
    assert simplify.edge_stats(dev(_oracle("s1_sphere", 16)["faces"])).closed
    for faces in (_plane()[1], np.array([[0, 1, 2], [0, 1, 2]], np.int32), np.array([[0, 1, 2], [2, 1, 0]], np.int32), np.zeros((0, 3), np.int32)):
        assert tuple(simplify.edge_stats(dev(faces))) == _np_edge_stats(faces)


# ---------------------------------------------------------------- GPU: the launch edges ----------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cells", FINE_CELLS)
@pytest.mark.parametrize("mesh", ["s1_sphere", "mario"])
def test_edge_finest_grids(mesh, cells):
    _fine_preconditions(mesh, cells)
    _both(mesh, cells)


@gpu
@pytest.mark.parametrize("cells", FINE_CELLS + [4])
def test_edge_corner_cells(cells):
    want = _corner_preconditions(cells)
    got = _both("corners", cells, UNIT01)
    assert got.clamped == _oracle("corners", cells, UNIT01, "mean")["clamped"] and tuple(got.faces.shape) == want["faces"].shape
    from tssplat_amd import simplify
    quadric = simplify.simplify(*(dev(x) for x in _corner_mesh()), cells, bounds=UNIT01)
    assert quadric.clamped == want["clamped"] and (cells != 1023 or quadric.clamped > 0)


@gpu
@pytest.mark.parametrize("mesh", BLOCK_MESHES)
def test_edge_block_sized_meshes(mesh):
    _block_preconditions(mesh)
    assert tuple(_both(mesh, BLOCK_CELLS).faces.shape)[0] > 0
    _both(mesh, 3, (-1.0, 1.0))


@gpu
def test_edge_dedupe_across_a_workgroup():
    v, f = _dedupe_boundary_mesh()
    order, _ = _sorted_survivors(v, f, DEDUPE_CELLS)
    assert order[255] == 255 and order[256] == 256
    got = _both("dedupe_boundary", DEDUPE_CELLS)
    assert got.duplicates == _oracle("s1_sphere", DEDUPE_CELLS)["duplicates"] + 1


# ---------------------------------------------------------------- GPU: end to end ----------------------------------------------------------------
@gpu
def test_merge_tets_simplify_clusters_the_extracted_surface():
    from tssplat_amd import merge, simplify
    v, e = (dev(x) for x in _two_spheres())
    plain = merge.merge_tets(v, e, grid=32, bounds=UNIT)
    off = merge.merge_tets(v, e, grid=32, bounds=UNIT, simplify=None)
    assert off.simplified is None and plain.simplified is None and off.closed == plain.closed and off.inside_fraction == plain.inside_fraction
    assert torch.equal(off.v.view(torch.int32), plain.v.view(torch.int32)) and torch.equal(off.faces, plain.faces)
    got = merge.merge_tets(v, e, grid=32, bounds=UNIT, simplify=2)
    s = got.simplified
    assert isinstance(s, simplify.SimplifiedSurface) and s.cells == 16 and s.bounds == UNIT and got.v is s.v and got.faces is s.faces
    assert 0 < got.faces.shape[0] < plain.faces.shape[0] and 0 < got.v.shape[0] < plain.v.shape[0]
    assert got.closed == simplify.edge_stats(got.faces).closed and (got.grid, got.inside_fraction, got.level) == (plain.grid, plain.inside_fraction, plain.level)
    # the clustering of the plain surface, bit for bit the oracle's
    want = SO.simplify(plain.v.cpu().numpy(), plain.faces.cpu().numpy(), 16, UNIT)
    _assert_equal(s, want, "merge_tets(simplify=2)")
    # containment: every vertex of the plain surface within sqrt(3) h of its cell's representative
    rep = want["cell_pos"][np.searchsorted(want["cell_keys"], want["vertex_keys"])].astype(np.float64)
    assert (np.linalg.norm(plain.v.cpu().numpy().astype(np.float64) - rep, axis=1) <= np.sqrt(3.0) * want["h"]).all()
    filled = merge.merge_tets(v, e, grid=32, bounds=UNIT, fill="outer", simplify=4)
    assert filled.fill == "outer" and filled.simplified.cells == 8 and 0 < filled.faces.shape[0] < got.faces.shape[0]
    with pytest.raises(RuntimeError, match="simplify must be None or an integer in 2"):
        merge.merge_tets(v, e, grid=32, bounds=UNIT, simplify=1)


@gpu
def test_renderer_export_merged_writes_the_simplified_mesh(tmp_path):
    from tssplat_amd import atlas, geometry, merge, renderers

    class Field(torch.nn.Module):
        def forward(self, positions):
            return {"color": 0.5 + 0.5 * torch.sin(torch.stack([3.0 * positions[..., 0] + 1.0, 4.0 * positions[..., 1], 5.0 * positions[..., 2] - 0.5], -1))}

    v, e = _two_spheres()
    geo = geometry.TetMeshGeometry(v, e, use_smooth_barrier=False, optimize_geo=False)
    merged = renderers.MeshRasterizer(geo, Field()).export_merged(str(tmp_path), "material", grid=32, simplify=2)
    out = tmp_path / "material"
    assert sorted(os.listdir(out)) == ["merged_surface.mtl", "merged_surface.obj", "merged_surface.png"]
    rv, rf, uv, uv_idx, tex = atlas.load_textured_obj(str(out), "merged_surface")
    want = merge.merge_tets(dev(v), dev(e), grid=32, simplify=2)
    assert merged.simplified is not None and merged.simplified.cells == 16
    assert rv.tobytes() == want.v.cpu().numpy().tobytes() == merged.v.cpu().numpy().tobytes()
    assert rf.tobytes() == want.faces.cpu().numpy().tobytes() and len(rf) < merge.merge_tets(dev(v), dev(e), grid=32).faces.shape[0]
    assert tex.shape == (1024, 1024, 3) and len(uv_idx) == len(rf)
    plain = geo.export_merged(str(tmp_path / "geo"), "final", grid=32, simplify=2)
    assert os.listdir(tmp_path / "geo") == ["final_merged.obj"] and torch.equal(plain.faces, want.faces)
