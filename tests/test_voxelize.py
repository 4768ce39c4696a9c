"""Voxelising triangle meshes (tssplat_amd/voxelize.py): the integer winding number on the merge's grid, the occupancy made of it and
volume IoU.  tests/voxel_oracle.py is the definition; the device results are compared with it bit for bit, counts included: no
tolerance.  The oracle itself is checked on the CPU against closed meshes whose inside is known, the algebra of the winding number
(reversal, addition, permutation) and the union field of the merge, which states the same inside by other means."""
import functools
import os

import numpy as np
import pytest
import torch

import union_oracle as U
import voxel_oracle as V
from tssplat_amd import _build, _capi, voxelize

gpu = pytest.mark.gpu
INVALID = 1     # TSAMD_ERR_INVALID_ARGUMENT
UNIT = (-1.0, 1.0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------- meshes ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    return np.ascontiguousarray(d["vertices"], dtype=np.float32), np.ascontiguousarray(d["faces"], dtype=np.int32)


def _node(G, index, bounds=UNIT):
    return bounds[0] + (index + 0.5) * (bounds[1] - bounds[0]) / G


def _box(lo, hi):
    """Twelve triangles, normals outwards."""
    v = np.array([[x, y, z] for x in (lo, hi) for y in (lo, hi) for z in (lo, hi)], dtype=np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return v, np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], dtype=np.int32)


def _octahedron(centre, radius):
    c = np.asarray(centre, dtype=np.float64)
    v = np.array([c + radius * np.eye(3)[a] * s for a in range(3) for s in (1, -1)], dtype=np.float32)       # +x -x +y -y +z -z
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    return v, np.array(f, dtype=np.int32)


def _hostile(G=16, bounds=UNIT):
    """One good triangle; six invalid faces (NaN, +inf, -inf, an index past the end, a negative index, a vertex at 10^9 h); two faces that are
    degenerate on every axis (a repeated corner, three collinear corners on the lattice)."""
    h = (bounds[1] - bounds[0]) / G
    v = np.array([[-0.5, -0.5, -0.5], [0.5, -0.4, -0.3], [-0.3, 0.6, 0.2], [np.nan, 0, 0], [np.inf, 0, 0], [-np.inf, 0, 0], [1e9 * h, 0, 0], [0, 0, 0],
                  [0.5, 0.5, 0.5]], dtype=np.float32)
    f = np.array([[0, 1, 2], [0, 1, 3], [0, 4, 2], [5, 1, 2], [0, 1, 9], [0, -1, 2], [0, 0, 1], [0, 7, 8], [0, 1, 6]], dtype=np.int32)
    return v, f


@functools.lru_cache(maxsize=None)
def _case(name):
    """``(v, faces, G, bounds)``."""
    s1 = _golden("s1_sphere")
    if name == "s1_sphere":
        return (*s1, 32, U.default_bounds(s1[0], 32))
    if name == "mario":
        m = _golden("mario_mesh")
        return (*m, 48, U.default_bounds(m[0], 48))
    if name == "box64":
        return (*_box(_node(64, 12), _node(64, 44)), 64, UNIT)
    if name == "box16":
        return (*_box(_node(16, 3), _node(16, 11)), 16, UNIT)
    if name == "octahedron":
        return (*_octahedron([_node(16, 8)] * 3, 5 * 0.125), 16, UNIT)
    if name == "hostile":
        return (*_hostile(), 16, UNIT)
    if name == "one_triangle":
        return np.array([[-0.7, -0.6, -0.2], [0.8, -0.5, 0.1], [-0.1, 0.9, 0.4]], dtype=np.float32), np.array([[0, 1, 2]], dtype=np.int32), 19, UNIT
    if name == "empty":
        return s1[0], np.zeros((0, 3), dtype=np.int32), 7, UNIT
    if name == "outside":
        return s1[0] + np.float32(5.0), s1[1], 17, UNIT
    if name == "half_outside":
        return s1[0] + np.array([1.0, 0.3, -0.2], dtype=np.float32), s1[1], 21, (-1.3, 1.3)
    if name == "smallest_grid":
        return (*s1, 1, (-1.1, 1.1))
    # ---- the launch edges (the section "launch edges" below states what each is for) ----
    if name.startswith("sphere_g"):
        return (*s1, int(name[len("sphere_g"):]), (-1.1, 1.1))
    if name == "span_triangle":
        return (*_span_triangle(), 129, UNIT)
    if name.startswith("half_outside_g"):
        return (*_case("half_outside")[:2], int(name[len("half_outside_g"):]), (-1.3, 1.3))
    if name.startswith("half_open_g"):
        return (*_half_open(), int(name[len("half_open_g"):]), (-1.3, 1.3))
    if name.startswith("split_axis"):
        return (*_split_mesh(int(name[len("split_axis"):])), NODE_GRID, NODE_BOUNDS)
    if name == "full_ballot":
        return (*_full_ballot_mesh(), NODE_GRID, NODE_BOUNDS)
    if name == "six_spheres":
        return (*_six_spheres(), 40, (-1.6, 1.6))
    if name == "lattice_limit":
        return (*_limit_mesh(False), 1, UNIT)
    if name == "past_the_limit":
        return (*_limit_mesh(True), 1, UNIT)
    raise KeyError(name)


def _span_triangle():
    """One open triangle across the cube (-1, 1): every column it covers stays open."""
    return np.array([[-0.9, -0.8, -0.7], [0.9, -0.7, 0.2], [-0.2, 0.95, 0.6]], dtype=np.float32), np.array([[0, 1, 2]], dtype=np.int32)


def _half_open():
    """``half_outside`` and one open triangle in the plane x + y + 3 z = 0 that leaves the cube (-1.3, 1.3) on every side: along i and along j
    its crossings run from before the first node to past the last one."""
    v, f = _case("half_outside")[:2]
    sheet = np.array([[40, -10, -10], [20, 10, -10], [-30, 0, 10]], dtype=np.float32)
    return np.concatenate([v, sheet]), np.concatenate([f, [[len(v), len(v) + 1, len(v) + 2]]]).astype(np.int32)


NODE_GRID, NODE_BOUNDS = 24, (0.0, 24.0)           # h = 1: a coordinate is a node index plus a fraction, column p has its centre at p + 0.5
SPLIT_BOXES = [(4, 4), (1, 16), (16, 1), (2, 8), (1, 17), (17, 1)]      # candidate columns along b x along c: four of LANE_COLUMNS, two of one more


def _world(axis, ray, b, c):
    p = [0.0, 0.0, 0.0]
    p[axis], p[(axis + 1) % 3], p[(axis + 2) % 3] = ray, b, c
    return p


def _split_mesh(axis):
    """Six single faces whose boxes of candidate columns, seen along ``axis``, are SPLIT_BOXES; every second one is reversed."""
    v, f = [], []
    for n, (nb, nc) in enumerate(SPLIT_BOXES):
        b0, c0 = 2 + n % 3, 1 + n % 2
        blo, bhi, clo, chi = b0 + 0.3, b0 + nb - 0.3, c0 + 0.2, c0 + nc - 0.4         # the centres b0 + 0.5 .. b0 + nb - 0.5 and no other
        plane = [(blo, clo), (bhi, clo), ((blo + bhi) / 2, chi)] if nc >= nb else [(blo, clo), (bhi, (clo + chi) / 2), (blo, chi)]
        rays = (5.3 + n, 7.7, 9.1 + 0.5 * n)
        v += [_world(axis, r, b, c) for r, (b, c) in zip(rays, plane)]
        f.append((3 * n, 3 * n + 1, 3 * n + 2) if n % 2 == 0 else (3 * n + 2, 3 * n + 1, 3 * n))
    return np.array(v, dtype=np.float32), np.array(f, dtype=np.int32)


FULL_BALLOT = range(64, 128)                       # the faces of wave 1 of workgroup 0


def _full_ballot_mesh():
    """130 faces in node units: those of FULL_BALLOT span 5.5 nodes on every axis (at least 5 x 5 candidate columns along each ray), the
    others 1.4 nodes (at most 2 x 2)."""
    rng = np.random.default_rng(64)
    v, f = [], []
    for n in range(130):
        o, size = rng.uniform(1.0, 17.0, 3), 5.5 if n in FULL_BALLOT else 1.4
        v += [o + [0, 0, size], o + [size, 0, 0], o + [0, size, 0]]
        f.append((3 * n, 3 * n + 1, 3 * n + 2) if n % 3 else (3 * n, 3 * n + 2, 3 * n + 1))
    return np.array(v, dtype=np.float32), np.array(f, dtype=np.int32)


def _six_spheres():
    """Six overlapping copies of the golden sphere, 0.45 along +-x, +-y, +-z; the one at +x is reversed."""
    v, f = _golden("s1_sphere")
    vs, fs = [], []
    for n, shift in enumerate([(0.45, 0, 0), (-0.45, 0, 0), (0, 0.45, 0), (0, -0.45, 0), (0, 0, 0.45), (0, 0, -0.45)]):
        vs.append(v + np.array(shift, dtype=np.float32))
        fs.append((f[:, ::-1] if n == 0 else f) + n * v.shape[0])
    return np.concatenate(vs), np.ascontiguousarray(np.concatenate(fs), dtype=np.int32)


# On G = 1 over (-1, 1): u = floor(512 (x + 1) + 0.5).  TOP and BOTTOM are the last usable coordinates, u = +-2^29; one float32 step of 2
# further out |u| is 2^29 + 1024
TOP, BOTTOM, PAST_TOP, PAST_BOTTOM = 1048575.0, -1048577.0, 1048577.0, -1048579.0
LIMIT_FACES = [                                     # corners on the limit on one, two and three axes; some cover the grid's one column
    [(BOTTOM, -0.5, -0.5), (TOP, -0.5, 0.25), (0.0, 0.75, 0.5)], [(BOTTOM, BOTTOM, 0.0), (TOP, BOTTOM, 0.5), (0.25, TOP, -0.5)],
    [(BOTTOM, BOTTOM, BOTTOM), (TOP, BOTTOM, TOP), (BOTTOM, TOP, TOP)], [(TOP, TOP, TOP), (BOTTOM, TOP, BOTTOM), (TOP, BOTTOM, BOTTOM)],
    [(TOP, 0.5, 0.5), (TOP, -0.5, BOTTOM), (0.5, TOP, 0.25)], [(3.0, 2.0, TOP), (TOP, 2.5, 4.0), (2.0, TOP, 3.0)],
    [(BOTTOM, 0.0, 0.0), (-0.5, BOTTOM, 0.5), (0.5, 0.5, BOTTOM)], [(TOP, TOP, 0.5), (BOTTOM, TOP, -0.5), (0.0, BOTTOM, BOTTOM)],
    [(TOP, BOTTOM, 0.25), (TOP, TOP, -0.25), (BOTTOM, 0.0, 0.0)], [(0.0, TOP, BOTTOM), (0.0, BOTTOM, BOTTOM), (0.25, 0.0, TOP)],
    [(BOTTOM, TOP, TOP), (TOP, TOP, BOTTOM), (BOTTOM, BOTTOM, BOTTOM)], [(-0.25, -0.5, TOP), (0.5, -0.25, TOP), (0.0, 0.5, BOTTOM)]]


def _limit_mesh(past):
    """The faces of LIMIT_FACES; with ``past`` each is followed by a copy whose first corner on the limit sits one step beyond it."""
    tris = []
    for tri in LIMIT_FACES:
        tris.append(tri)
        if past:
            flat = [x for p in tri for x in p]
            at = next(i for i, x in enumerate(flat) if x in (TOP, BOTTOM))
            flat[at] = PAST_TOP if flat[at] == TOP else PAST_BOTTOM
            tris.append([tuple(flat[0:3]), tuple(flat[3:6]), tuple(flat[6:9])])
    v = np.array([p for tri in tris for p in tri], dtype=np.float32)
    return v, np.arange(v.shape[0], dtype=np.int32).reshape(-1, 3)


def _candidate_boxes(name, axis):
    """``(nb, nc)`` int64 per face: the columns whose centre p S + S / 2 lies within the corners' range on the two plane axes, clipped to the
    grid (the module text of tests/voxel_oracle.py, written out with a ceiling and a floor).  Every face must be valid."""
    v, f, G, bounds = _case(name)
    u, _, usable = V.lattice(v, G, bounds)
    assert usable[f].all()
    out = []
    for x in ((axis + 1) % 3, (axis + 2) % 3):
        first = np.maximum(-((V.S // 2 - u[f, x].min(1)) // V.S), 0)              # ceil((min - S/2) / S)
        last = np.minimum((u[f, x].max(1) - V.S // 2) // V.S, G - 1)
        out.append(np.maximum(last - first + 1, 0))
    return out[0], out[1]


@functools.lru_cache(maxsize=None)
def _slab_deposits(name, axis):
    """How many columns have a deposit left at each of the G + 1 slabs."""
    v, f, G, bounds = _case(name)
    return (V.deposits(v, f, G, bounds, axis)["dep"] != 0).sum(axis=(1, 2))


CASES = ["s1_sphere", "mario", "box64", "octahedron", "hostile", "one_triangle", "empty", "outside", "half_outside", "smallest_grid"]


@functools.lru_cache(maxsize=None)
def _want_winding(name, axis):
    v, f, G, bounds = _case(name)
    return V.winding(v, f, G, bounds, axis)


@functools.lru_cache(maxsize=None)
def _want_occupancy(name, rule, rays):
    v, f, G, bounds = _case(name)
    per = [_want_winding(name, axis) for axis in range(rays)]              # V.occupancy, from the shared windings
    bits = [V.apply_rule(p["w"], rule) for p in per]
    votes = sum(b.astype(np.int32) for b in bits)
    return {"occ": bits[0] if rays == 1 else votes >= 2, "disputed": 0 if rays == 1 else int(((votes == 1) | (votes == 2)).sum()),
            "open_columns": tuple(p["open_columns"] for p in per), "invalid_faces": per[0]["invalid_faces"],
            "degenerate_faces": tuple(p["degenerate_faces"] for p in per), "deposits": tuple(p["deposits"] for p in per),
            "wave_faces": sum(p["wave_faces"] for p in per)}


@functools.lru_cache(maxsize=None)
def _two_sphere_merge(G, bounds=None):
    """tests/test_merge.py's two overlapping spheres (its ``_overlapping(2)``) merged by the oracle, on the merge's default bounds unless given."""
    import test_merge
    return U.merge_tets(*test_merge._overlapping(2), G, bounds)


# ---------------------------------------------------------------- CPU: the oracle ----------------------------------------------------------------
def test_oracle_sphere_is_closed_on_every_axis_and_has_the_meshs_volume():
    v, f, G, bounds = _case("s1_sphere")
    h = (bounds[1] - bounds[0]) / G
    volume = U.signed_mesh_volume(v, f)
    assert volume > 0
    for axis in range(3):
        w = _want_winding("s1_sphere", axis)
        assert w["open_columns"] == 0 and w["invalid_faces"] == 0
        assert set(np.unique(w["w"])) == {0, 1}
        assert abs(int((w["w"] != 0).sum()) * h ** 3 - volume) <= 0.02 * volume         # the staircase of a 32^3 grid


def test_oracle_box_and_octahedron_on_nodes_close_exactly():
    v, f, G, bounds = _case("box16")
    for axis in range(3):
        w = V.winding(v, f, G, bounds, axis)
        assert w["open_columns"] == 0 and w["degenerate_faces"] == 8 and w["invalid_faces"] == 0
        assert int((w["w"] != 0).sum()) == 512 and set(np.unique(w["w"])) == {0, 1}
        idx = np.argwhere(w["w"] != 0)                                                    # an 8^3 block: each tie goes to one of the two faces
        assert np.array_equal(idx.max(0) - idx.min(0), [7, 7, 7]) and idx.min() >= 3 and idx.max() <= 11
    for axis in range(3):
        w = _want_winding("octahedron", axis)
        assert w["open_columns"] == 0 and set(np.unique(w["w"])) == {0, 1} and w["w"][8, 8, 8] == 1


def test_oracle_reversal_addition_and_permutation():
    v, f, G, bounds = _case("s1_sphere")
    rng = np.random.default_rng(7)
    shift_a, shift_b = np.array([-0.21, 0.05, 0.0], dtype=np.float32), np.array([0.26, -0.11, 0.13], dtype=np.float32)
    big = (-1.5, 1.5)
    for axis in range(3):
        w = _want_winding("s1_sphere", axis)["w"]
        assert np.array_equal(V.winding(v, f[:, ::-1], G, bounds, axis)["w"], -w)
        assert np.array_equal(V.winding(v, f[rng.permutation(f.shape[0])], G, bounds, axis)["w"], w)
        wa, wb = V.winding(v + shift_a, f, G, big, axis), V.winding(v + shift_b, f, G, big, axis)
        both = V.winding(np.concatenate([v + shift_a, v + shift_b]), np.concatenate([f, f + v.shape[0]]), G, big, axis)
        assert np.array_equal(both["w"], wa["w"] + wb["w"]) and set(np.unique(both["w"])) == {0, 1, 2}
        assert both["open_columns"] == 0 and both["deposits"] == wa["deposits"] + wb["deposits"]


@pytest.mark.parametrize("G", [16, 24])
def test_oracle_round_trip_through_the_merge(G):
    """The merged surface is the level set of the union field, so voxelising it on the merge's own grid and bounds must give the field's
    own occupancy back at every node, along every axis."""
    m = _two_sphere_merge(G)
    inside = U.occupancy(m["field"], m["level"])
    assert m["closed"] and inside.any()
    for axis in range(3):
        w = V.winding(m["v"], m["faces"], G, m["bounds"], axis)
        assert w["open_columns"] == 0 and w["invalid_faces"] == 0 and set(np.unique(w["w"])) == {0, 1}
        assert np.array_equal(w["w"] != 0, inside), (axis, int(((w["w"] != 0) != inside).sum()))
    finer = V.occupancy(m["v"], m["faces"], G + 7, m["bounds"])
    assert finer["open_columns"] == (0, 0, 0)
    assert finer["disputed"] <= 0.01 * int(finer["occ"].sum())


@pytest.mark.parametrize("G", [16, 24])
def test_oracle_round_trip_differs_only_at_nodes_on_the_surface(G):
    """On the cube (-1, 1) the same scene puts nodes ON the surface: the field there is 10^-9, the level -h 2^-20, and the float32 vertex
    of the merged mesh next to such a node cannot say on which side of it the surface passes.  These are the ties the module text names:
    a node may differ from the field's occupancy only where the field is within h 2^-16 of the level, and no column opens."""
    m = _two_sphere_merge(G, UNIT)
    inside = U.occupancy(m["field"], m["level"])
    h = 2.0 / G
    for axis in range(3):
        w = V.winding(m["v"], m["faces"], G, UNIT, axis)
        differs = (w["w"] != 0) != inside
        assert w["open_columns"] == 0 and differs.sum() <= 8
        assert (np.abs(m["field"][differs].astype(np.float64) - float(m["level"])) <= h * 2.0 ** -16).all()


def test_oracle_mario_shows_its_defects_and_the_vote_contains_them():
    v, f = _golden("mario_mesh")
    G = 32
    bounds = U.default_bounds(v, G)
    per = [V.winding(v, f, G, bounds, axis) for axis in range(3)]
    vote = V.occupancy(v, f, G, bounds, "nonzero", 3)
    assert any(p["open_columns"] for p in per) and vote["open_columns"] == tuple(p["open_columns"] for p in per)
    for p in per:
        odd = int(((p["w"] != 0) & (p["w"] != 1)).sum())
        assert int(((p["w"] != 0) != vote["occ"]).sum()) < odd + 2 * G * p["open_columns"]     # an open column spoils at most its own G nodes


def test_oracle_hostile_mesh_counts():
    v, f, G, bounds = _case("hostile")
    for axis in range(3):
        w = _want_winding("hostile", axis)
        assert w["invalid_faces"] == 6 and w["degenerate_faces"] == 2
        assert w["deposits"] > 0 and w["open_columns"] == w["deposits"]                   # one open triangle: every covered column stays open
    occ = V.occupancy(v, f, G, bounds, "odd", 3)
    assert occ["invalid_faces"] == 6 and occ["degenerate_faces"] == (2, 2, 2)


def test_oracle_iou_of_a_sphere_and_its_half():
    v, f, G, bounds = _case("s1_sphere")
    r = V.mesh_volume_iou(v, f, v * np.float32(0.5), f, G, bounds)
    assert r["inside_b"] < r["inside_a"] and abs(r["iou"] - 0.125) <= 0.02                 # (1/2)^3 up to the staircase of both surfaces
    assert V.mesh_volume_iou(v, f, v, f, G, bounds)["iou"] == 1.0


# ---------------------------------------------------------------- CPU: the launch edges are reached ----------------------------------------------------------------
# Each fixture below exists for one edge of csrc/voxel_kernels.hip.  These tests state, on the oracle alone, that the fixture reaches
# its edge; the GPU tests of the same name further down compare the device with the oracle at it.
CARRY_GRIDS = [63, 64, 65, 127, 128, 129, 192]      # voxel_row_kernel scans the G + 1 slabs of a k-ray 64 per trip
TAIL_GRIDS = list(range(9, 17))                      # voxel_walk_kernel loads eight slabs per trip: every G % 8


def _carried(name):
    """How many k-rays carry a sum that is not 0 into the second and into the third trip of voxel_row_kernel: w at slabs 63 and 127."""
    w = _want_winding(name, 2)["w"]
    return tuple(int((w[:, :, s] != 0).sum()) if w.shape[2] > s else 0 for s in (63, 127))


@pytest.mark.parametrize("G", CARRY_GRIDS)
def test_edge_row_scan_carry_is_reached(G):
    """The carry into trip 2 is w at slab 63, the carry into trip 3 w at slab 127.  Up to G = 65 the sphere has closed by slab 63 and the
    sizes test where slab G falls (lane 63 of trip 1 at G = 63, a trip of its own at G = 64); from 127 on the carry is not 0, and at
    192 neither is the carry of the carry."""
    second, third = _carried(f"sphere_g{G}")
    print(f"G={G}: k-rays with w != 0 at slab 63: {second}, at slab 127: {third}")
    assert (second > 0) == (G >= 127) and (third > 0) == (G == 192)       # 129: three trips, but nothing is carried into the third
    assert second > 10000 or G <= 65
    assert third > 10000 or G < 192
    for axis in range(3):
        assert _want_winding(f"sphere_g{G}", axis)["open_columns"] == 0


def test_edge_open_triangle_carries_through_every_trip():
    """Three trips at G = 129 with a sum that never returns to 0: the carry into trips 2 and 3 and the lane of slab G all see it."""
    assert min(_carried("span_triangle")) > 0
    assert tuple(_want_winding("span_triangle", axis)["open_columns"] for axis in range(3)) == (3005, 3573, 6404)
    for axis in range(3):
        assert _want_winding("span_triangle", axis)["open_columns"] == _want_winding("span_triangle", axis)["deposits"]


def _tails_are_reached(G):
    for axis in (0, 1):
        sphere, sheet = _slab_deposits(f"half_outside_g{G}", axis), _slab_deposits(f"half_open_g{G}", axis)
        print(f"G={G} axis {axis}: columns with a deposit at slabs 0, G - 1, G: sphere {sphere[[0, G - 1, G]].tolist()}, with the sheet {sheet[[0, G - 1, G]].tolist()}; "
              f"open columns {_want_winding(f'half_open_g{G}', axis)['open_columns']}")
        assert sphere[G] > 0 and _want_winding(f"half_outside_g{G}", axis)["open_columns"] == 0
        assert sheet[0] > 0 and sheet[G - 1] > 0 and sheet[G] > 0 and _want_winding(f"half_open_g{G}", axis)["open_columns"] > 0


@pytest.mark.parametrize("G", TAIL_GRIDS)
def test_edge_walk_tails_are_reached(G):
    """Along i and j.  The closed sphere that leaves the cube deposits at slab G, the clamp of ceil(x) at the far end, and can open no
    column and reach no slab before its own first crossing; with the open sheet added there are deposits at slab 0 (the clamp at the
    near end), at slab G - 1, at slab G, and open columns."""
    _tails_are_reached(G)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_edge_sixteen_column_split_is_reached(axis):
    """Boxes of exactly LANE_COLUMNS columns go down the lane path, boxes of one more down the wave path; 1 x n and n x 1 boxes are the
    column arithmetic q / nc, q % nc at nc = 1 and at nb = 1."""
    name = f"split_axis{axis}"
    nb, nc = _candidate_boxes(name, axis)
    assert list(zip(nb.tolist(), nc.tolist())) == SPLIT_BOXES and V.LANE_COLUMNS == 16
    want = _want_winding(name, axis)
    assert want["wave_faces"] == sum(b * c == 17 for b, c in SPLIT_BOXES) == 2 and want["invalid_faces"] == want["degenerate_faces"] == 0
    v, f, G, bounds = _case(name)
    for n, (b, c) in enumerate(SPLIT_BOXES):                              # face by face: which path, and that it deposits at all
        alone = V.deposits(v, f[n:n + 1], G, bounds, axis)
        assert alone["wave_faces"] == (b * c > 16) and 0 < alone["deposits"] <= b * c


def test_edge_wave_walks_are_reached():
    """The sphere at G = 127: about half of the faces are wave faces, every wave holds both kinds, wave faces fall in all four waves of a
    workgroup and the last workgroup is partial.  full_ballot: all 64 lanes of one wave hold a wave face."""
    f = _case("sphere_g127")[1]
    assert f.shape[0] % 256 not in (0, 255)
    for axis in range(3):
        nb, nc = _candidate_boxes("sphere_g127", axis)
        big = nb * nc > V.LANE_COLUMNS
        assert int(big.sum()) == _want_winding("sphere_g127", axis)["wave_faces"] and 1400 < big.sum() < 1600
        assert all(0 < big[s:s + 64].sum() < min(64, f.shape[0] - s) for s in range(0, f.shape[0], 64))
        assert all(max(big[s:s + 64].sum() for s in range(64 * wave, f.shape[0], 256)) > 8 for wave in range(4))
        nb, nc = _candidate_boxes("full_ballot", axis)
        assert np.array_equal(np.nonzero(nb * nc > V.LANE_COLUMNS)[0], np.asarray(FULL_BALLOT)) and (nb * nc > 0).all()
        assert _want_winding("full_ballot", axis)["wave_faces"] == 64


def test_edge_replica_wrap_is_reached():
    """71 deposit workgroups add to 64 copies of the counts; the scene also has w outside {0, 1}, where the three rules part."""
    v, f, G, bounds = _case("six_spheres")
    assert f.shape[0] == 17976 and (f.shape[0] + 255) // 256 == 71 > 64
    for axis in range(3):
        assert {-1, 2} <= set(np.unique(_want_winding("six_spheres", axis)["w"]).tolist())
    occ = [_want_occupancy("six_spheres", rule, 3)["occ"] for rule in V.RULES]
    assert all((occ[a] != occ[b]).any() for a, b in ((0, 1), (0, 2), (1, 2)))


def _covers_exactly(corners, axis, p, q):
    """Coverage of column (p, q) by the face with the lattice corners ``corners`` (three triples of Python integers), by the rule in
    the module text of tests/voxel_oracle.py, in arbitrary-precision integers.  None: degenerate along this axis."""
    b, c = (axis + 1) % 3, (axis + 2) % 3
    (Ab, Ac), (Bb, Bc), (Cb, Cc) = ((int(k[b]), int(k[c])) for k in corners)
    area = (Bb - Ab) * (Cc - Ac) - (Bc - Ac) * (Cb - Ab)
    if area == 0:
        return None
    sg = 1 if area > 0 else -1
    Pb, Pc = p * V.S + V.S // 2, q * V.S + V.S // 2

    def inner(Qb, Qc, Rb, Rc):
        e, db, dc = sg * ((Rb - Qb) * (Pc - Qc) - (Rc - Qc) * (Pb - Qb)), sg * (Rb - Qb), sg * (Rc - Qc)
        return e > 0 or (e == 0 and (db > 0 or (db == 0 and dc > 0)))

    return inner(Bb, Bc, Cb, Cc) and inner(Cb, Cc, Ab, Ac) and inner(Ab, Ac, Bb, Bc)


def test_edge_lattice_limit_is_reached():
    """|u| = 2^29 is usable and one step further is not; at the limit the int64 products of the oracle (and of the kernel) still equal
    the products of unbounded integers."""
    u, _, usable = V.lattice(np.array([[TOP, BOTTOM, 0.0], [PAST_TOP, 0.0, 0.0], [0.0, PAST_BOTTOM, 0.0]], dtype=np.float32), 1, UNIT)
    assert usable.tolist() == [True, False, False] and u[0].tolist() == [1 << 29, -(1 << 29), 512] and V.U_MAX == 1 << 29
    v, f, G, bounds = _case("lattice_limit")
    u, _, usable = V.lattice(v, G, bounds)
    assert usable.all()
    on_limit = (np.abs(u[f]) == V.U_MAX).any(axis=1).sum(axis=1)           # per face: on how many axes a corner sits on the limit
    assert {1, 2, 3} <= set(on_limit.tolist()) and on_limit.min() >= 1
    for axis in range(3):
        exact = [_covers_exactly([[int(x) for x in u[i]] for i in face], axis, 0, 0) for face in f.tolist()]
        want = _want_winding("lattice_limit", axis)
        print(f"axis {axis}: {exact.count(True)} faces cover the column, {exact.count(False)} do not, {exact.count(None)} are degenerate")
        assert want["deposits"] == exact.count(True) > 0 and exact.count(False) > 0 and want["degenerate_faces"] == exact.count(None)
        assert want["invalid_faces"] == 0
        past = _want_winding("past_the_limit", axis)
        assert past["invalid_faces"] == len(LIMIT_FACES) and past["deposits"] == want["deposits"] and np.array_equal(past["w"], want["w"])


# ---------------------------------------------------------------- CPU: argument checks ----------------------------------------------------------------
def test_c_abi_workspace_bytes_and_argument_errors_launch_nothing():
    """Every argument error is reported before anything touches the device: all device pointers here are null or made up."""
    lib = _capi.load()
    p = 0x1000                                                            # "not null"; never dereferenced on these paths
    assert lib.tsamd_voxel_workspace_bytes(1) == 6144 + 3 * 2 * 4 and lib.tsamd_voxel_workspace_bytes(512) == 6144 + 3 * 513 * 512 * 512 * 4
    assert lib.tsamd_voxel_workspace_bytes(0) == -1 and lib.tsamd_voxel_workspace_bytes(513) == -1

    def wind(v=p, nv=8, faces=p, nt=4, grid=8, lo=-1.0, hi=1.0, axis=0, ws=p, w=p, stats=p):
        return lib.tsamd_voxel_winding(v, nv, faces, nt, grid, lo, hi, axis, ws, w, stats, None)

    def occ(v=p, nv=8, faces=p, nt=4, grid=8, lo=-1.0, hi=1.0, rule=0, rays=3, ws=p, out=p, stats=p):
        return lib.tsamd_voxel_occupancy(v, nv, faces, nt, grid, lo, hi, rule, rays, ws, out, stats, None)

    nan = float("nan")
    cases = [(fn, kw, word) for fn in (wind, occ) for kw, word in [
        (dict(grid=0), "grid"), (dict(grid=513), "grid"), (dict(grid=-4), "grid"), (dict(nv=-1), "n_vertices"), (dict(nv=1 << 31), "n_vertices"),
        (dict(nt=-1), "n_triangles"), (dict(nt=1 << 31), "n_triangles"), (dict(lo=1.0, hi=1.0), "lo"), (dict(lo=2.0), "lo"), (dict(hi=nan), "lo"),
        (dict(lo=-float("inf")), "lo"), (dict(v=None), "v_dev"), (dict(faces=None), "faces_dev"), (dict(ws=None), "workspace_dev"),
        (dict(stats=None), "stats_out_dev"), (dict(stats=p + 4), "stats_out_dev"), (dict(ws=p + 4), "workspace_dev"), (dict(v=p + 1), "v_dev")]]
    cases += [(wind, dict(axis=3), "axis"), (wind, dict(axis=-1), "axis"), (wind, dict(w=None), "w_out_dev"), (wind, dict(w=p + 2), "w_out_dev"),
              (occ, dict(rule=3), "rule"), (occ, dict(rule=-1), "rule"), (occ, dict(rays=2), "rays"), (occ, dict(rays=0), "rays"), (occ, dict(out=None), "occ_out_dev"),
              (wind, dict(nt=0, v=None, faces=None, w=None), "w_out_dev"), (occ, dict(nt=0, v=None, faces=None, ws=None), "workspace_dev")]
    for fn, kw, word in cases:
        assert fn(**kw) == INVALID, (fn.__name__, kw)
        msg = lib.tsamd_last_error().decode()
        assert msg and word in msg, (fn.__name__, kw, msg)


def test_python_arguments_are_checked_by_name():
    """Nothing here reaches the library: a CPU tensor is refused first, with the argument's name."""
    from tssplat_amd import spheres_init
    v, f = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32)
    for call, word in [(lambda: voxelize.winding(v, f, 8, UNIT), "v must be a GPU"), (lambda: voxelize.occupancy(v, f, 8, UNIT), "v must be a GPU"),
                       (lambda: voxelize.winding(v, f, 0, UNIT), "grid"), (lambda: voxelize.winding(v, f, 513, UNIT), "grid"),
                       (lambda: voxelize.winding(v, f, 8, (1.0, 1.0)), "bounds"), (lambda: voxelize.winding(v, f, 8, UNIT, axis=3), "axis"),
                       (lambda: voxelize.occupancy(v, f, 8, UNIT, rule="even"), "rule"), (lambda: voxelize.occupancy(v, f, 8, UNIT, rays=2), "rays"), (lambda: voxelize.occupancy(v, f, 8, UNIT, rays=3.0), "rays"),
                       (lambda: voxelize.occupancy(v.double(), f, 8, UNIT), "v must be float32"), (lambda: voxelize.occupancy(v, f.long(), 8, UNIT), "faces must be int32"),
                       (lambda: voxelize.occupancy(v, f[:, :2], 8, UNIT), "faces must be"), (lambda: voxelize.mesh_volume_iou(v, f, v, f, 8, UNIT), "v_a"),
                       (lambda: voxelize.mesh_volume_iou(v, f, v, f, 8, UNIT, rule=0), "rule"),
                       (lambda: spheres_init.cover_occupancy(torch.zeros(4, 4, 4, dtype=torch.bool), 3), "occ")]:
        with pytest.raises(RuntimeError, match=word):
            call()
    assert voxelize.workspace_bytes(7) == 6144 + 3 * 8 * 49 * 4 and voxelize.LANE_COLUMNS == V.LANE_COLUMNS and voxelize.SUBCELL_BITS == V.SUBCELL_BITS
    assert tuple(voxelize.RULES) == V.RULES


def test_build_lists_carry_the_voxel_sources():
    assert {"voxel_kernels.hip", "voxel_capi.cpp"} <= set(_build.SOURCES) and "voxel.h" in _build.HEADERS
    assert _build.SOURCE_FLAGS["voxel_kernels.hip"] == ["-ffp-contract=off"]
    for name in ("voxel_kernels.hip", "voxel_capi.cpp", "voxel.h"):
        assert os.path.exists(os.path.join(_build.CSRC, name))


# ---------------------------------------------------------------- GPU: bit for bit ----------------------------------------------------------------
@gpu
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("name", CASES)
def test_winding_equals_oracle(name, axis):
    v, f, G, bounds = _case(name)
    want = _want_winding(name, axis)
    got = voxelize.winding(dev(v), dev(f), G, bounds, axis)
    assert got.w.dtype == torch.int32 and tuple(got.w.shape) == (G, G, G)
    assert np.array_equal(got.w.cpu().numpy(), want["w"]), int((got.w.cpu().numpy() != want["w"]).sum())
    assert (got.open_columns, got.invalid_faces, got.degenerate_faces, got.deposits, got.wave_faces) == \
        (want["open_columns"], want["invalid_faces"], want["degenerate_faces"], want["deposits"], want["wave_faces"])
    if name == "box64":                                                   # 32 x 32 columns per face: no lane walks that, a wave did
        assert got.wave_faces == 4 and got.deposits == 2 * 32 * 32
    if name == "s1_sphere":
        assert got.wave_faces == 0 and got.deposits > 0                  # ... and here every face went down the lane path
    if name in ("empty", "outside"):
        assert got.deposits == 0 and not got.w.any()


@gpu
@pytest.mark.parametrize("rays", [1, 3])
@pytest.mark.parametrize("rule", V.RULES)
@pytest.mark.parametrize("name", CASES)
def test_occupancy_equals_oracle(name, rule, rays):
    v, f, G, bounds = _case(name)
    want = _want_occupancy(name, rule, rays)
    got = voxelize.occupancy(dev(v), dev(f), G, bounds, rule, rays)
    assert got.occ.dtype == torch.bool and tuple(got.occ.shape) == (G, G, G)
    assert np.array_equal(got.occ.cpu().numpy(), want["occ"]), int((got.occ.cpu().numpy() != want["occ"]).sum())
    assert (got.open_columns, got.disputed, got.invalid_faces, got.degenerate_faces, got.deposits, got.wave_faces) == \
        (want["open_columns"], want["disputed"], want["invalid_faces"], want["degenerate_faces"], want["deposits"], want["wave_faces"])
    assert got.occ.view(torch.uint8).max().item() <= 1                    # a bool tensor made of bytes 0 and 1 only


@gpu
def test_results_are_repeatable():
    v, f, G, bounds = _case("mario")
    dv, df = dev(v), dev(f)
    a, b = voxelize.winding(dv, df, G, bounds, 2), voxelize.winding(dv, df, G, bounds, 2)
    assert torch.equal(a.w, b.w) and _counts(a) == _counts(b)
    oa, ob = voxelize.occupancy(dv, df, G, bounds), voxelize.occupancy(dv, df, G, bounds)
    assert torch.equal(oa.occ, ob.occ) and _counts(oa) == _counts(ob)


def _counts(record):
    import dataclasses
    return tuple(getattr(record, f.name) for f in dataclasses.fields(record) if f.name not in ("w", "occ"))


@gpu
def test_device_round_trip_through_the_merge():
    from tssplat_amd import merge
    import test_merge
    v, e = test_merge._overlapping(2)
    m = merge.merge_tets(dev(v), dev(e), 24)                               # the scene and bounds of test_oracle_round_trip_through_the_merge
    field = merge.union_field(dev(v), dev(e), 24, m.bounds)
    got = voxelize.occupancy(m.v, m.faces, m.grid, m.bounds)
    assert got.open_columns == (0, 0, 0) and got.disputed == 0 and got.invalid_faces == 0
    assert torch.equal(got.occ, merge.occupancy(field, m.level)) and got.occ.any()
    for axis in range(3):
        assert torch.equal(voxelize.winding(m.v, m.faces, m.grid, m.bounds, axis).w != 0, got.occ)


@gpu
def test_mesh_volume_iou():
    v, f, G, bounds = _case("s1_sphere")
    dv, df = dev(v), dev(f)
    same = voxelize.mesh_volume_iou(dv, df, dv, df, G, bounds)
    assert same["iou"] == 1.0 and same["inside_a"] == same["inside_b"] == int(_want_occupancy("s1_sphere", "nonzero", 3)["occ"].sum())
    half = voxelize.mesh_volume_iou(dv, df, dev(v * np.float32(0.5)), df, G, bounds)
    want = V.mesh_volume_iou(v, f, v * np.float32(0.5), f, G, bounds)
    assert abs(want["iou"] - 0.125) <= 0.02                               # the staircase margin, measured by the oracle ...
    assert (half["iou"], half["inside_a"], half["inside_b"]) == (want["iou"], want["inside_a"], want["inside_b"])        # ... and met exactly
    assert half["a"].open_columns == (0, 0, 0) and half["b"].invalid_faces == 0
    auto = voxelize.mesh_volume_iou(dv, df, dev(v * np.float32(0.5)), df, grid=G)       # bounds=None: default_bounds over both vertex sets
    assert auto["bounds"] == bounds and auto["iou"] == want["iou"]


@gpu
def test_cover_occupancy_is_the_tail_of_init_spheres():
    from tssplat_amd import spheres_init
    import test_spheres_init as T
    alpha, mvp = T._hull_scene(1, 24, 40)
    a, m = dev(alpha), dev(mvp)
    G, n = 33, 5
    want = spheres_init.init_spheres(a, m, n, grid=G, threshold=T.THRESHOLD, channel=1, min_radius=0.02)
    hull = spheres_init.visual_hull(a, m, grid=G, threshold=T.THRESHOLD, channel=1)
    got = spheres_init.cover_occupancy(hull, n, (-1.0, 1.0), min_radius=0.02)
    assert len(want) >= 1 and got.pt.tobytes() == want.pt.tobytes() and got.r.tobytes() == want.r.tobytes()
    assert got.hull_fraction == want.hull_fraction and got.uncovered_fraction == want.uncovered_fraction
    with pytest.raises(ValueError, match="cover_occupancy"):
        spheres_init.cover_occupancy(torch.ones(4, 4, 4, dtype=torch.bool, device="cuda"), 2)


@gpu
def test_key_point_of_a_voxelised_sphere_is_its_centre():
    from tssplat_amd import spheres_init
    import spheres_init_oracle as O
    v, f = _golden("s1_sphere")
    G, bounds = 33, (-1.25, 1.25)
    occ = voxelize.occupancy(dev(v), dev(f), G, bounds)
    kp = spheres_init.cover_occupancy(occ.occ, 1, bounds)
    want = V.occupancy(v, f, G, bounds)["occ"]
    flat, q, _ = O.greedy_cover(want, O.distance_transform_sq(want), 1, bounds)
    pt, r = O.centres_and_radii(flat, q, G, bounds)
    assert len(kp) == 1 and kp.pt.tobytes() == pt.tobytes() and kp.r.tobytes() == r.tobytes()
    assert np.array_equal(np.unravel_index(int(flat[0]), (G, G, G)), (16, 16, 16)) and np.array_equal(kp.pt[0], O.voxel_centres(G, bounds)[[16, 16, 16]])
    assert 0.85 < float(kp.r[0]) / 0.92 <= 1.0                             # the inscribed ball of a unit sphere, up to a voxel


@gpu
def test_geometry_volume_iou_on_two_spheres():
    from tssplat_amd import geometry
    import test_merge
    v, e = test_merge._overlapping(2)
    geo = geometry.TetMeshGeometry(v, e, use_smooth_barrier=False)
    sv, sf = geo.tet_v.detach()[geo.surface_vid.long()].contiguous(), geo.surface_fid.contiguous()
    same = geo.volume_iou(sv, sf, grid=24)
    assert same["iou"] == 1.0 and same["inside_a"] > 0 and same["a"].open_columns == (0, 0, 0)
    ball = _golden("s1_sphere")
    other = geo.volume_iou(dev(ball[0] * np.float32(0.4) + np.array([-0.2, 0.05, 0.0], dtype=np.float32)), dev(ball[1]), grid=24, bounds=UNIT)
    want = V.mesh_volume_iou(sv.cpu().numpy(), sf.cpu().numpy(), ball[0] * np.float32(0.4) + np.array([-0.2, 0.05, 0.0], dtype=np.float32), ball[1], 24, UNIT)
    assert other["iou"] == want["iou"] and 0.3 < other["iou"] < 0.8       # one of the two balls, roughly


# ---------------------------------------------------------------- GPU: the launch edges ----------------------------------------------------------------
def _winding_equals_oracle(name, axis):
    v, f, G, bounds = _case(name)
    want = _want_winding(name, axis)
    got = voxelize.winding(dev(v), dev(f), G, bounds, axis)
    w = got.w.cpu().numpy()
    assert w.dtype == np.int32 and w.shape == (G, G, G)
    assert np.array_equal(w, want["w"]), (name, axis, int((w != want["w"]).sum()))
    assert (got.open_columns, got.invalid_faces, got.degenerate_faces, got.deposits, got.wave_faces) == \
        (want["open_columns"], want["invalid_faces"], want["degenerate_faces"], want["deposits"], want["wave_faces"]), (name, axis)
    return got


def _occupancy_equals_oracle(name, rule, rays):
    v, f, G, bounds = _case(name)
    want = _want_occupancy(name, rule, rays)
    got = voxelize.occupancy(dev(v), dev(f), G, bounds, rule, rays)
    occ = got.occ.cpu().numpy()
    assert occ.dtype == np.bool_ and occ.shape == (G, G, G) and got.occ.view(torch.uint8).max().item() <= 1
    assert np.array_equal(occ, want["occ"]), (name, rule, rays, int((occ != want["occ"]).sum()))
    assert (got.open_columns, got.disputed, got.invalid_faces, got.degenerate_faces, got.deposits, got.wave_faces) == \
        (want["open_columns"], want["disputed"], want["invalid_faces"], want["degenerate_faces"], want["deposits"], want["wave_faces"]), (name, rule, rays)
    return got


@gpu
@pytest.mark.parametrize("G", CARRY_GRIDS)
def test_edge_row_scan_carry(G):
    """test_edge_row_scan_carry_is_reached states what each size reaches."""
    name = f"sphere_g{G}"
    second, third = _carried(name)
    assert (second > 0) == (G >= 127) and (third > 0) == (G == 192)
    for axis in range(3):
        _winding_equals_oracle(name, axis)
    for rule in V.RULES:
        _occupancy_equals_oracle(name, rule, 3)


@gpu
def test_edge_open_triangle_carries_through_every_trip_on_the_device():
    assert min(_carried("span_triangle")) > 0
    got = [_winding_equals_oracle("span_triangle", axis) for axis in range(3)]
    assert tuple(g.open_columns for g in got) == (3005, 3573, 6404)
    for rule in V.RULES:
        assert _occupancy_equals_oracle("span_triangle", rule, 3).open_columns == (3005, 3573, 6404)


@gpu
@pytest.mark.parametrize("G", TAIL_GRIDS)
def test_edge_walk_tails(G):
    _tails_are_reached(G)
    for name in (f"half_outside_g{G}", f"half_open_g{G}"):
        for axis in (0, 1):
            _winding_equals_oracle(name, axis)
        for rule in V.RULES:
            for rays in (1, 3):
                _occupancy_equals_oracle(name, rule, rays)


@gpu
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_edge_sixteen_column_split(axis):
    name = f"split_axis{axis}"
    nb, nc = _candidate_boxes(name, axis)
    assert list(zip(nb.tolist(), nc.tolist())) == SPLIT_BOXES
    got = _winding_equals_oracle(name, axis)
    assert got.wave_faces == 2 and got.deposits > 0
    _occupancy_equals_oracle(name, "nonzero", 3)
    if axis == 0:
        _occupancy_equals_oracle(name, "odd", 1)


@gpu
def test_edge_wave_walks():
    """sphere_g127 itself runs in test_edge_row_scan_carry; here the counts the wave path produces are named."""
    for axis in range(3):
        got = _winding_equals_oracle("sphere_g127", axis)
        assert 1400 < got.wave_faces < 1600
        got = _winding_equals_oracle("full_ballot", axis)
        nb, nc = _candidate_boxes("full_ballot", axis)
        assert got.wave_faces == 64 == int((nb * nc > V.LANE_COLUMNS).sum())
    for rule in V.RULES:
        assert _occupancy_equals_oracle("full_ballot", rule, 3).wave_faces == 3 * 64


@gpu
def test_edge_replica_wrap():
    for axis in range(3):
        got = _winding_equals_oracle("six_spheres", axis)
        assert int(got.w.min()) <= -1 and int(got.w.max()) >= 2
    occ = []
    for rule in V.RULES:
        occ.append(_occupancy_equals_oracle("six_spheres", rule, 3).occ)
        _occupancy_equals_oracle("six_spheres", rule, 1)
    assert not torch.equal(occ[0], occ[1]) and not torch.equal(occ[0], occ[2]) and not torch.equal(occ[1], occ[2])


@gpu
def test_edge_lattice_limit():
    """test_edge_lattice_limit_is_reached checks the oracle's coverage at |u| = 2^29 with unbounded integers; the device must agree with it."""
    for axis in range(3):
        assert _winding_equals_oracle("lattice_limit", axis).invalid_faces == 0
        assert _winding_equals_oracle("past_the_limit", axis).invalid_faces == len(LIMIT_FACES)
    for rule in V.RULES:
        for rays in (1, 3):
            _occupancy_equals_oracle("lattice_limit", rule, rays)
            assert _occupancy_equals_oracle("past_the_limit", rule, rays).invalid_faces == len(LIMIT_FACES)
