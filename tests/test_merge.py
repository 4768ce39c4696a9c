"""Merging tet-spheres into one closed surface (tssplat_amd/merge.py): the union field, the marching-tetrahedra extraction and the
exports built on them.  The device results are compared with tests/union_oracle.py bit for bit: no tolerance.  The oracle itself
is checked on the CPU against exact rational arithmetic, a plane distance computed another way and the properties of a closed
mesh."""
import functools
import itertools
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import union_oracle as U
from tssplat_amd import _build, _capi, scenes

gpu = pytest.mark.gpu
INVALID = 1     # TSAMD_ERR_INVALID_ARGUMENT
UNIT = (-1.0, 1.0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------- scenes ----------------------------------------------------------------
def _two_spheres(k, c0, r0, c1, r1):
    bv, bt = scenes.kuhn_ball(k)
    bv = bv / np.linalg.norm(bv, axis=1).max()
    v = np.concatenate([bv * r0 + np.asarray(c0), bv * r1 + np.asarray(c1)]).astype(np.float32)
    return v, np.concatenate([bt, bt + bv.shape[0]]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _overlapping(k):
    return _two_spheres(k, [-0.2, 0.05, 0.0], 0.4, [0.25, -0.1, 0.1], 0.35)


@functools.lru_cache(maxsize=None)
def _disjoint(k):
    return _two_spheres(k, [-0.5, 0.0, 0.0], 0.3, [0.5, 0.0, 0.0], 0.3)


@functools.lru_cache(maxsize=None)
def _merged(kind, k, G, level=None):
    v, e = (_overlapping if kind == "overlapping" else _disjoint)(k)
    return U.merge_tets(v, e, G, UNIT, level)


ONE_TET_V = np.array([[-0.5, -0.4, -0.45], [0.6, -0.3, -0.5], [-0.2, 0.7, -0.35], [0.1, 0.05, 0.65]], dtype=np.float32)
ONE_TET = np.array([[0, 1, 2, 3]], dtype=np.int32)


def _random_field(G, seed, border_outside):
    f = np.random.default_rng(seed + G).standard_normal((G, G, G)).astype(np.float32)
    if border_outside:
        f[0], f[-1], f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1] = -1, -1, -1, -1, -1, -1
    return f


# ---------------------------------------------------------------- CPU: the oracle ----------------------------------------------------------------
def _det3(u, v, w):
    return u[0] * (v[1] * w[2] - v[2] * w[1]) - u[1] * (v[0] * w[2] - v[2] * w[0]) + u[2] * (v[0] * w[1] - v[1] * w[0])


def _rational_side(tet, p):
    """+1 strictly inside, 0 on the boundary, -1 outside: exact (integers as Fractions), for a tet of positive volume."""
    a, b, c, d = ([Fraction(int(x)) for x in q] for q in tet)
    p = [Fraction(x) for x in p]
    sub = lambda q, o: [x - y for x, y in zip(q, o)]
    # the signed volumes of (p, b, c, d), (a, p, c, d), (a, b, p, d), (a, b, c, p)
    vols = [_det3(sub(b, p), sub(c, p), sub(d, p)), _det3(sub(p, a), sub(c, a), sub(d, a)), _det3(sub(b, a), sub(p, a), sub(d, a)),
            _det3(sub(b, a), sub(c, a), sub(p, a))]
    if any(x < 0 for x in vols):
        return -1
    return 0 if any(x == 0 for x in vols) else 1


def test_oracle_sign_convention_is_kuhn_balls():
    v, e = scenes.kuhn_ball(2)
    p = v.astype(np.float32).astype(np.float64)
    for tet in e:
        assert U.signed_volume(*p[tet]) > 0
    # oracle/tet_energy_oracle.py's rest volume is det(Dm) / 6 with Dm's columns b - a, c - a, d - a: the same sign
    from oracle import tet_energy_oracle as TE
    Dm = TE.rest_operators(v.astype(np.float32), e)[0]
    assert (np.linalg.det(Dm) > 0).all()


def test_oracle_inside_decision_equals_exact_rational_arithmetic():
    """Small-integer tets on a grid whose nodes are the integers 0 .. 7 (h = 1): strictly inside <=> f > 0, strictly outside <=>
    f < 0, on the boundary |f| is rounding noise, and f > default level <=> inside or on the boundary."""
    G, bounds = 8, (-0.5, 7.5)
    assert np.array_equal(U.node_positions(G, bounds), np.arange(8.0))
    level = U.default_level(G, bounds)
    rng = np.random.default_rng(5)
    seen = {-1: 0, 0: 0, 1: 0}
    done = 0
    while done < 12:
        tet = rng.integers(0, 8, size=(4, 3))
        if _det3(tet[1] - tet[0], tet[2] - tet[0], tet[3] - tet[0]) <= 0:
            continue
        done += 1
        f = U.union_field(tet.astype(np.float32), ONE_TET, G, bounds)
        lo, hi = tet.min(0), tet.max(0)
        for i, j, k in itertools.product(range(G), repeat=3):
            in_box = all(lo[a] - 1 <= x <= hi[a] + 1 for a, x in enumerate((i, j, k)))
            if not in_box:
                assert f[i, j, k] == -np.inf
                continue
            side = _rational_side(tet, (i, j, k))
            seen[side] += 1
            value = float(f[i, j, k])
            assert (value > 0 if side > 0 else value < 0 if side < 0 else abs(value) < 1e-12), (tet, (i, j, k), side, value)
            assert (f[i, j, k] > level) == (side >= 0), (tet, (i, j, k), side, value)
    assert min(seen.values()) > 20


def test_oracle_values_equal_a_plane_distance_computed_another_way():
    """The oracle's float64 field, before its rounding to float32, against min over the faces of (p - q) . n with numpy's cross
    and norm and a geometric sign test: every covered node to 1e-12 relative to the coordinates' magnitude, which is 1 here (relative
    to the value itself no rounded sum can be held near the surface, where the value passes through 0).  The float32 field is that
    one rounded, nothing else."""
    rng = np.random.default_rng(11)
    G = 9
    c = U.node_positions(G, UNIT)
    P = np.stack(np.meshgrid(c, c, c, indexing="ij"), -1)
    checked = 0
    for _ in range(8):
        tet = rng.uniform(-0.9, 0.9, size=(4, 3)).astype(np.float32)
        p = tet.astype(np.float64)
        vol = np.linalg.det(p[1:] - p[0])
        if vol < 0:
            tet, p, vol = tet[[0, 2, 1, 3]], p[[0, 2, 1, 3]], -vol
        if vol < 0.05:
            continue
        checked += 1
        f = U.union_field_f64(tet, ONE_TET, G, UNIT)
        want = np.full((G, G, G), np.inf)
        for opp in range(4):
            face = p[[x for x in range(4) if x != opp]]
            n = np.cross(face[1] - face[0], face[2] - face[0])
            n = n / np.linalg.norm(n)
            if n @ (p[opp] - face[0]) < 0:
                n = -n
            want = np.minimum(want, (P - face[0]) @ n)
        covered = np.isfinite(f)
        assert covered.sum() > 50 and (np.abs(want[covered]) < 0.05).any()          # nodes near the surface are among them
        assert (np.abs(f[covered] - want[covered]) <= 1e-12).all()
        rounded = U.union_field(tet, ONE_TET, G, UNIT)
        assert rounded.dtype == np.float32 and np.array_equal(rounded, f.astype(np.float32))
    assert checked >= 4


def _tet_codes(inside):
    """{(permutation index, 4-bit pattern of the chain's corners)} over all cubes."""
    G = inside.shape[0]
    out = set()
    for pi, perm in enumerate(U.PERMS):
        masks = [0, U.AXIS_BIT[perm[0]], U.AXIS_BIT[perm[0]] | U.AXIS_BIT[perm[1]], 7]
        code = np.zeros((G - 1,) * 3, dtype=np.int32)
        for x, m in enumerate(masks):
            di, dj, dk = (m >> 2) & 1, (m >> 1) & 1, m & 1
            code |= inside[di:G - 1 + di, dj:G - 1 + dj, dk:G - 1 + dk].astype(np.int32) << x
        out |= {(pi, int(cd)) for cd in np.unique(code)}
    return out


@pytest.mark.parametrize("G", [5, 9])
def test_oracle_extraction_of_random_signs_is_closed_and_oriented(G):
    f = _random_field(G, 0, border_outside=True)
    v, faces, closed = U.extract_surface(f, UNIT, 0.0)
    assert closed and len(faces) > 0
    if G == 9:         # all 14 mixed patterns of every one of the six tets, and every one of the seven edge types, occur
        assert {(pi, cd) for pi in range(6) for cd in range(1, 15)} <= _tet_codes(f > 0)
        inside = f > 0
        for m in range(1, 8):
            di, dj, dk = (m >> 2) & 1, (m >> 1) & 1, m & 1
            assert (inside[:G - di, :G - dj, :G - dk] != inside[di:, dj:, dk:]).any()
    assert U.edge_defects(faces) == 0                  # every undirected edge in exactly two triangles, once each way
    assert np.isfinite(v).all() and faces.min() == 0 and faces.max() == len(v) - 1 and len(np.unique(faces)) == len(v)
    assert U.signed_mesh_volume(v, faces) > 0
    # a border node inside: not closed
    g = f.copy()
    g[0, 2, 2] = 1
    assert not U.extract_surface(g, UNIT, 0.0)[2]


def _cube_counts(inside):
    G = inside.shape[0]
    corners = [inside[di:G - 1 + di, dj:G - 1 + dj, dk:G - 1 + dk] for di in (0, 1) for dj in (0, 1) for dk in (0, 1)]
    return int(np.logical_and.reduce(corners).sum()), int(np.logical_or.reduce(corners).sum())


@pytest.mark.parametrize("kind,G,chi", [("overlapping", 17, 2), ("overlapping", 24, 2), ("disjoint", 17, 4)])
def test_oracle_two_sphere_scenes(kind, G, chi):
    m = _merged(kind, 3, G)
    v, faces, field = m["v"], m["faces"], m["field"]
    assert m["closed"] and U.edge_defects(faces) == 0
    assert U.euler_characteristic(len(v), faces) == chi
    # the divergence theorem against cube counts: the surface passes only through cubes with corners of both signs
    h = 2.0 / G
    full, touched = _cube_counts(U.occupancy(field, m["level"]))
    vol = U.signed_mesh_volume(v, faces)
    assert vol > 0 and full > 0 and h ** 3 * full <= vol <= h ** 3 * touched, (h ** 3 * full, vol, h ** 3 * touched)
    # the extraction never interpolates a -inf: an inside node's neighbours lie in the dilated box of the tet that contains it
    inside = U.occupancy(field, m["level"])
    for mask in range(1, 8):
        di, dj, dk = (mask >> 2) & 1, (mask >> 1) & 1, mask & 1
        a, b = (slice(0, G - di), slice(0, G - dj), slice(0, G - dk)), (slice(di, G), slice(dj, G), slice(dk, G))
        change = inside[a] != inside[b]
        assert change.any() and np.isfinite(field[a][change]).all() and np.isfinite(field[b][change]).all()
    assert (field.astype(np.float64) != float(m["level"])).all()         # no node sits exactly on the level
    assert m["inside_fraction"] == inside.sum() / G ** 3


def test_oracle_level_zero_opens_a_cavity_and_the_default_level_closes_it():
    """Nodes on faces shared by two tets inside the solid read exactly 0 from both: at level 0 they are outside."""
    at0, dflt = _merged("disjoint", 3, 17, 0.0), _merged("disjoint", 3, 17)
    zeros = at0["field"] == 0
    assert zeros.sum() == 20 and U.occupancy(dflt["field"], dflt["level"])[zeros].all() and not U.occupancy(at0["field"], 0.0)[zeros].any()
    assert U.edge_defects(at0["faces"]) == 0 and U.euler_characteristic(len(at0["v"]), at0["faces"]) == 8    # two spurious components
    assert U.euler_characteristic(len(dflt["v"]), dflt["faces"]) == 4
    assert dflt["level"] == float(np.float32(-(2.0 / 17) * 2.0 ** -20)) and dflt["level"] < 0


def test_oracle_default_bounds_leave_two_nodes_of_margin():
    v, _ = _overlapping(2)
    for G in (5, 17, 128):
        lo, hi = U.default_bounds(v, G)
        h = (hi - lo) / G
        c = U.node_positions(G, (lo, hi))
        mn, mx = float(v.min()), float(v.max())
        assert c[1] < mn and mx < c[-2]                               # two nodes outside the vertices on both sides
        assert abs((mn - lo) - 2 * h) < 1e-12 and abs((hi - mx) - 2 * h) < 1e-12
    with pytest.raises(ValueError):
        U.default_bounds(v, 4)


def test_volume_iou_oracle():
    a = np.zeros((3, 3, 3), dtype=bool)
    b = a.copy()
    assert U.volume_iou(a, b) == 1.0
    a[0], b[:2] = True, True
    assert U.volume_iou(a, b) == 9 / 18


# ---------------------------------------------------------------- CPU: argument checks ----------------------------------------------------------------
def test_c_abi_argument_errors_launch_nothing():
    """Every argument error is reported before anything touches the device: all device pointers here are null or made up."""
    lib = _capi.load()
    p = 0x1000                                                            # "not null"; never dereferenced on these paths

    def field(tet_v=p, nv=8, elem=p, nt=4, grid=8, lo=-1.0, hi=1.0, out=p):
        return lib.tsamd_union_field(tet_v, nv, elem, nt, grid, lo, hi, out, None)

    def count(f=p, grid=8, level=0.0, vmask=p, vcount=p, tcount=p, flag=p):
        return lib.tsamd_surface_count(f, grid, level, vmask, vcount, tcount, flag, None)

    def emit(f=p, grid=8, lo=-1.0, hi=1.0, level=0.0, vmask=p, voff=p, toff=p, nv=3, nt=1, v=p, faces=p):
        return lib.tsamd_surface_emit(f, grid, lo, hi, level, vmask, voff, toff, nv, nt, v, faces, None)

    nan = float("nan")
    cases = [
        (field, dict(grid=1), "grid"), (field, dict(grid=513), "grid"), (field, dict(grid=-4), "grid"), (field, dict(nv=-1), "n_vertices"),
        (field, dict(nt=-1), "n_tets"), (field, dict(nt=(1 << 30) + 1), "n_tets"), (field, dict(lo=1.0, hi=1.0), "lo"), (field, dict(lo=2.0), "lo"),
        (field, dict(hi=nan), "lo"), (field, dict(lo=-float("inf")), "lo"), (field, dict(tet_v=None), "tet_v_dev"), (field, dict(elem=None), "elem_dev"),
        (field, dict(out=None), "field_out_dev"), (field, dict(nt=0, tet_v=None, elem=None, out=None), "field_out_dev"),
        (count, dict(grid=1), "grid"), (count, dict(grid=513), "grid"), (count, dict(level=nan), "level"), (count, dict(f=None), "field_dev"),
        (count, dict(vmask=None), "vmask_out_dev"), (count, dict(vcount=None), "vcount_out_dev"), (count, dict(tcount=None), "tcount_out_dev"),
        (count, dict(flag=None), "open_out_dev"),
        (emit, dict(grid=1), "grid"), (emit, dict(grid=513), "grid"), (emit, dict(lo=1.0, hi=-1.0), "lo"), (emit, dict(level=nan), "level"),
        (emit, dict(nv=-1), "n_vertices"), (emit, dict(nt=-1), "n_triangles"), (emit, dict(nv=7 * 512 + 1), "n_vertices"),
        (emit, dict(nt=12 * 512 + 1), "n_triangles"), (emit, dict(f=None), "field_dev"), (emit, dict(vmask=None), "vmask_dev"),
        (emit, dict(voff=None), "voffset_dev"), (emit, dict(toff=None), "toffset_dev"), (emit, dict(v=None), "v_out_dev"),
        (emit, dict(faces=None), "faces_out_dev"),
    ]
    for fn, kw, word in cases:
        assert fn(**kw) == INVALID, (fn.__name__, kw)
        msg = lib.tsamd_last_error().decode()
        assert msg and word in msg, (fn.__name__, kw, msg)
    assert emit(nv=0, nt=0, v=None, faces=None) == 0                     # nothing to write: nothing is launched


def test_python_arguments_are_checked_by_name():
    """Nothing here reaches the library: a CPU tensor is refused first, with the argument's name."""
    from tssplat_amd import merge
    v, e, f = torch.zeros(4, 3), torch.zeros(1, 4, dtype=torch.int32), torch.zeros(4, 4, 4)
    for call, word in [(lambda: merge.union_field(v, e, 8, UNIT), "tet_v"), (lambda: merge.merge_tets(v, e), "tet_v"),
                       (lambda: merge.merge_tets(np.zeros((4, 3), np.float32), e), "tet_v"), (lambda: merge.extract_surface(f, UNIT, 0.0), "field"),
                       (lambda: merge.occupancy(f, 0.0), "field"), (lambda: merge.default_bounds(v, 8), "tet_v"), (lambda: merge.default_bounds(v, 4), "grid"),
                       (lambda: merge.default_level(1, UNIT), "grid"), (lambda: merge.default_level(513, UNIT), "grid"),
                       (lambda: merge.default_level(8, (1.0, 1.0)), "bounds"), (lambda: merge.volume_iou(f, f), "a must be a bool"),
                       (lambda: merge.volume_iou(f > 0, f), "b must be a bool"), (lambda: merge.volume_iou(f > 0, f[:2] > 0), "b must have")]:
        with pytest.raises(RuntimeError, match=word):
            call()
    assert merge.default_level(17, UNIT) == float(U.default_level(17, UNIT))
    assert merge.volume_iou(torch.zeros(2, 2, 2, dtype=torch.bool), torch.zeros(2, 2, 2, dtype=torch.bool)) == 1.0


def test_build_lists_carry_the_merge_sources():
    assert {"merge_kernels.hip", "merge_capi.cpp"} <= set(_build.SOURCES) and "merge.h" in _build.HEADERS
    assert _build.SOURCE_FLAGS["merge_kernels.hip"] == ["-ffp-contract=off"]
    for name in ("merge_kernels.hip", "merge_capi.cpp", "merge.h"):
        assert os.path.exists(os.path.join(_build.CSRC, name))


# ---------------------------------------------------------------- GPU: the field ----------------------------------------------------------------
def _field_both(tet_v, elem, G, bounds=UNIT, want=None):
    from tssplat_amd import merge
    if want is None:
        want = U.union_field(tet_v, elem, G, bounds)
    got = merge.union_field(dev(np.asarray(tet_v, np.float32).reshape(-1, 3)), dev(np.asarray(elem, np.int32).reshape(-1, 4)), G, bounds)
    assert got.dtype == torch.float32 and tuple(got.shape) == (G, G, G)
    got = got.cpu().numpy()
    assert got.tobytes() == want.tobytes(), (int((got != want).sum()), float(np.nanmax(np.abs(np.where(np.isfinite(got) & np.isfinite(want), got - want, 0)))))
    return want


@gpu
def test_field_of_one_tet():
    assert U.signed_volume(*ONE_TET_V.astype(np.float64)) > 0
    want = _field_both(ONE_TET_V, ONE_TET, 5)
    assert (want > 0).any() and (want < 0).any()
    small = _field_both(ONE_TET_V * np.float32(0.4) - np.float32(0.3), ONE_TET, 5)      # its dilated box leaves nodes uncovered
    assert (small == -np.inf).any() and np.isfinite(small).any()


@gpu
def test_inverted_and_flat_tets_contribute_nothing():
    for v, e in [(ONE_TET_V, ONE_TET[:, [0, 2, 1, 3]]), (ONE_TET_V * np.float32([1, 1, 0]), ONE_TET), (ONE_TET_V[[0, 1, 1, 3]], ONE_TET),
                 (ONE_TET_V, np.zeros((0, 4), np.int32))]:
        want = _field_both(v, e, 5)
        assert (want == -np.inf).all()


@gpu
def test_bad_indices_and_nan_coordinates_are_skipped():
    v, e = _overlapping(1)
    v, e = v.copy(), e.copy()
    clean = U.union_field(v, e, 9, UNIT)
    n = v.shape[0]
    nan_v = np.concatenate([v, np.float32([[np.nan, 0, 0], [0, np.inf, 0]])])
    extra = np.array([[0, 1, 2, n + 2], [0, 1, 2, -1], [2 ** 31 - 1, 1, 2, 3], [0, 1, 2, n], [0, 1, n + 1, 3]], dtype=np.int32)   # bad, bad, bad, NaN, inf
    want = _field_both(nan_v, np.concatenate([extra[:2], e, extra[2:]]), 9)
    assert want.tobytes() == clean.tobytes()                             # the neighbours are intact


@gpu
def test_one_tet_spanning_the_whole_grid():
    v = np.float32([[-5, -5, -5], [20, -5, -5], [-5, 20, -5], [-5, -5, 20]])
    assert U.signed_volume(*v.astype(np.float64)) > 0
    want = _field_both(v, ONE_TET, 33)
    assert (want > 0).all()


@gpu
def test_a_tet_half_outside_the_bounds():
    v = ONE_TET_V + np.float32([0.9, 0.8, -0.7])
    want = _field_both(v, ONE_TET, 9)
    assert (want[-1] > 0).any() and (want == -np.inf).any()
    far = _field_both(ONE_TET_V + np.float32([5, 0, 0]), ONE_TET, 9)      # wholly outside: an empty box
    assert (far == -np.inf).all()
    _field_both(ONE_TET_V, ONE_TET, 9, bounds=(-0.3, 0.2))                 # the grid inside the tet's box


@gpu
@pytest.mark.parametrize("G", [17, 65])
def test_field_of_two_overlapping_spheres_and_repeatable(G):
    from tssplat_amd import merge
    v, e = _overlapping(2)
    _field_both(v, e, G)
    a = merge.union_field(dev(v), dev(e), G, UNIT).cpu().numpy()
    b = merge.union_field(dev(v), dev(e), G, UNIT).cpu().numpy()
    assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- GPU: the extraction ----------------------------------------------------------------
def _extract_both(field, level, bounds=UNIT):
    from tssplat_amd import merge
    wv, wf, wc = U.extract_surface(field, bounds, level)
    v, faces, closed = merge.extract_surface(dev(field), bounds, level)
    assert v.dtype == torch.float32 and faces.dtype == torch.int32 and isinstance(closed, bool)
    assert tuple(v.shape) == wv.shape and tuple(faces.shape) == wf.shape, (tuple(v.shape), wv.shape, tuple(faces.shape), wf.shape)
    assert closed == wc
    assert v.cpu().numpy().tobytes() == wv.tobytes() and faces.cpu().numpy().tobytes() == wf.tobytes()
    return wv, wf, wc


@gpu
@pytest.mark.parametrize("border_outside", [True, False])
@pytest.mark.parametrize("G", [5, 9])
def test_extraction_of_random_signs_equals_oracle(G, border_outside):
    v, faces, closed = _extract_both(_random_field(G, 0, border_outside), 0.0)
    assert closed == border_outside and len(faces) > 0
    _extract_both(_random_field(G, 1, border_outside), 0.25, bounds=(-0.3, 1.7))


@gpu
def test_extraction_with_exact_level_values_nans_and_infinities():
    G, level = 9, 0.25
    rng = np.random.default_rng(3)
    f = (np.round(rng.standard_normal((G, G, G)) * 4) / 4).astype(np.float32)
    assert (f == level).sum() > 20
    special = rng.permutation(G ** 3)[:60]
    f.reshape(-1)[special[:20]] = np.nan
    f.reshape(-1)[special[20:40]] = np.inf
    f.reshape(-1)[special[40:]] = -np.inf
    v, faces, _ = _extract_both(f, level)
    assert np.isfinite(v).all() and len(faces) > 0
    p = v[faces]
    assert (np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1) == 0).any()    # f_b == level: degenerate triangles


@gpu
@pytest.mark.parametrize("G", [2, 5])
def test_extraction_of_constant_fields_and_one_corner_node(G):
    v, faces, closed = _extract_both(np.full((G, G, G), -1, np.float32), 0.0)
    assert len(v) == 0 and len(faces) == 0 and closed
    v, faces, closed = _extract_both(np.full((G, G, G), 1, np.float32), 0.0)
    assert len(v) == 0 and len(faces) == 0 and not closed
    for corner in [(0, 0, 0), (G - 1, G - 1, G - 1), (0, G - 1, 0)]:
        f = np.full((G, G, G), -1, np.float32)
        f[corner] = 1
        v, faces, closed = _extract_both(f, 0.0)
        assert len(v) > 0 and len(faces) > 0 and not closed


# ---------------------------------------------------------------- GPU: end to end ----------------------------------------------------------------
def _read_plain_obj(path):
    v, f = [], []
    for line in open(path):
        w = line.split()
        if w and w[0] == "v":
            v.append([float(x) for x in w[1:4]])
        elif w and w[0] == "f":
            f.append([int(x) - 1 for x in w[1:4]])
    return np.asarray(v, np.float32).reshape(-1, 3), np.asarray(f, np.int32).reshape(-1, 3)


@gpu
@pytest.mark.parametrize("bounds,level", [(None, None), (UNIT, 0.0)])
def test_merge_tets_equals_oracle(bounds, level):
    from tssplat_amd import merge
    v, e = _overlapping(2)
    want = U.merge_tets(v, e, 17, bounds, level)
    got = merge.merge_tets(dev(v), dev(e), grid=17, bounds=bounds, level=level)
    assert isinstance(got, merge.MergedSurface) and got.grid == 17
    assert got.bounds == want["bounds"] and got.level == want["level"] and got.closed is True and want["closed"]
    assert got.inside_fraction == want["inside_fraction"] and 0 < got.inside_fraction < 1
    assert got.v.cpu().numpy().tobytes() == want["v"].tobytes() and got.faces.cpu().numpy().tobytes() == want["faces"].tobytes()
    assert U.edge_defects(want["faces"]) == 0 and U.euler_characteristic(len(want["v"]), want["faces"]) == 2
    occ = merge.occupancy(merge.union_field(dev(v), dev(e), 17, got.bounds), got.level)
    assert occ.dtype == torch.bool and np.array_equal(occ.cpu().numpy(), U.occupancy(want["field"], want["level"]))
    other = torch.roll(occ, 1, 0)
    assert merge.volume_iou(occ, occ) == 1.0 and merge.volume_iou(occ, other) == U.volume_iou(occ.cpu().numpy(), other.cpu().numpy()) < 1.0


@gpu
def test_geometry_export_merged_writes_the_merged_mesh(tmp_path):
    from tssplat_amd import geometry
    v, e = _overlapping(2)
    geo = geometry.TetMeshGeometry(v, e, use_smooth_barrier=False)
    merged = geo.export_merged(str(tmp_path / "out"), "final", grid=17)
    want = U.merge_tets(v, e, 17)
    assert os.listdir(tmp_path / "out") == ["final_merged.obj"] and merged.closed
    rv, rf = _read_plain_obj(tmp_path / "out" / "final_merged.obj")
    assert rv.tobytes() == want["v"].tobytes() == merged.v.cpu().numpy().tobytes()
    assert rf.tobytes() == want["faces"].tobytes() == merged.faces.cpu().numpy().tobytes()
    fixed = geo.export_merged(str(tmp_path / "out"), "fixed", grid=9, bounds=UNIT)
    assert fixed.bounds == UNIT and fixed.v.cpu().numpy().tobytes() == U.merge_tets(v, e, 9, UNIT)["v"].tobytes()


@gpu
def test_renderer_export_merged_bakes_the_material(tmp_path):
    from tssplat_amd import atlas, geometry, renderers

    class Field(torch.nn.Module):
        def forward(self, positions):
            return {"color": 0.5 + 0.5 * torch.sin(torch.stack([3.0 * positions[..., 0] + 1.0, 4.0 * positions[..., 1], 5.0 * positions[..., 2] - 0.5], -1))}

    v, e = _overlapping(2)
    geo = geometry.TetMeshGeometry(v, e, use_smooth_barrier=False, optimize_geo=False)
    ren = renderers.MeshRasterizer(geo, Field())
    merged = ren.export_merged(str(tmp_path), "material", grid=17)
    out = tmp_path / "material"
    assert sorted(os.listdir(out)) == ["merged_surface.mtl", "merged_surface.obj", "merged_surface.png"]
    rv, rf, uv, uv_idx, tex = atlas.load_textured_obj(str(out), "merged_surface")
    want = U.merge_tets(v, e, 17)
    assert rv.tobytes() == want["v"].tobytes() and rf.tobytes() == want["faces"].tobytes()
    R = 1024                                                             # the smallest power of two >= 1024 that holds the triangles
    assert tex.shape == (R, R, 3) and atlas.atlas_layout(len(rf), R)
    assert np.array_equal(uv, atlas.atlas_uv(len(rf), R)[0].numpy()) and np.array_equal(uv_idx, atlas.atlas_uv(len(rf), R)[1].numpy())
    positions, owner = atlas.bake_positions(merged.v, merged.faces, R)
    owned = (owner >= 0).cpu().numpy()
    colour = Field()(positions)["color"].cpu().numpy()
    stored = np.rint(tex * 255).astype(np.uint8)
    assert owned.sum() > 10000 and np.array_equal(stored[owned], atlas.texture_to_image(colour)[::-1][owned])
    assert not stored[~owned].any()
    with pytest.raises(AssertionError):
        renderers.MeshRasterizer(geo).export_merged(str(tmp_path), "none")


# ---------------------------------------------------------------- edges: lattice tets, exact ties and box limits on nodes ----------------------------------------------------------------
# Random float corners never put a node exactly on a face plane, give two tets exactly the same value at a node, or put a box limit
# (mn - lo) / h - 0.5 on an exact integer.  Tets with corners on grid nodes do all three: the bounds (-0.5, G - 0.5) make h = 1 and the
# node positions the integers 0 .. G - 1, so every coordinate, difference and cross product below is an exact integer in float64.
def _lattice_bounds(G):
    return (-0.5, G - 0.5)


@functools.lru_cache(maxsize=None)
def _kuhn_block(step):
    """The 48 Kuhn tets of a 2 x 2 x 2 block of cubes whose edges are `step` node steps long, with a corner on node (0, 0, 0):
    (corners int64 [27, 3], elem int32 [48, 4]), every tet of positive volume."""
    v = np.stack(np.meshgrid(*[np.arange(3)] * 3, indexing="ij"), -1).reshape(-1, 3) * step
    elem = []
    for origin in itertools.product(range(2), repeat=3):
        for perm in U.PERMS:
            chain = [np.array(origin)]
            for ax in perm:
                chain.append(chain[-1] + np.eye(3, dtype=np.int64)[ax])
            ids = [int((c[0] * 3 + c[1]) * 3 + c[2]) for c in chain]
            if U.perm_sign(perm) < 0:
                ids[2], ids[3] = ids[3], ids[2]
            elem.append(ids)
    return v.astype(np.int64), np.asarray(elem, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def _random_lattice_tets(count=400, seed=7):
    """`count` random tets of positive volume with corners on the nodes 0 .. 7: (corners int64 [4 count, 3], elem int32 [count, 4])."""
    rng = np.random.default_rng(seed)
    tets = []
    while len(tets) < count:
        tet = rng.integers(0, 8, size=(4, 3))
        vol = _det3(tet[1] - tet[0], tet[2] - tet[0], tet[3] - tet[0])
        if vol != 0:
            tets.append(tet if vol > 0 else tet[[0, 2, 1, 3]])
    return np.concatenate(tets).astype(np.int64), np.arange(4 * count, dtype=np.int32).reshape(-1, 4)


# On grid 48 the fixture is repeated at these node offsets (the same on all three axes), so that the first and the last plane of a
# tet's box -- its smallest node coordinate - 1 and its largest + 1 -- fall on the planes 14, 15, 16, 17 around the slab seam at 16, and
# on 31 and 32 around the next one.
LATTICE = {"kuhn2": (lambda: _kuhn_block(2), (11, 12, 15, 16, 27, 28, 31, 32)), "kuhn4": (lambda: _kuhn_block(4), (9, 10, 11, 12, 13, 14, 26, 27, 28, 29)),
           "random": (_random_lattice_tets, (10, 13, 26, 29)), "sparse": (lambda: _random_lattice_tets(96), (10, 13, 26, 29))}
SEAM_PLANES = {14, 15, 16, 17, 31, 32}


@functools.lru_cache(maxsize=None)
def _lattice_tets(name, G):
    make, offsets = LATTICE[name]
    v, elem = make()
    if G == 8:
        return v.astype(np.float32), elem
    assert G == 48
    return (np.concatenate([v + o for o in offsets]).astype(np.float32), np.concatenate([elem + n * len(v) for n in range(len(offsets))]).astype(np.int32))


@functools.lru_cache(maxsize=None)
def _lattice_field(name, G):
    return U.union_field(*_lattice_tets(name, G), G, _lattice_bounds(G))


def _per_tet_minima(tet_v, elem, G):
    """float64 [T, G, G, G]: each tet's own min over its four faces, -inf outside its box."""
    return np.stack([U.union_field_f64(tet_v, elem[t:t + 1], G, _lattice_bounds(G)) for t in range(len(elem))])


@pytest.mark.parametrize("name", sorted(LATTICE))
def test_edge_lattice_tets_are_reached(name):
    G = 8
    tet_v, elem = _lattice_tets(name, G)
    assert np.array_equal(U.node_positions(G, _lattice_bounds(G)), np.arange(8.0)) and (tet_v == np.round(tet_v)).all()
    assert all(U.tet_contributes(tet_v, tet) for tet in elem)
    f = U.union_field_f64(tet_v, elem, G, _lattice_bounds(G))
    per = _per_tet_minima(tet_v, elem, G)
    assert np.array_equal(per.max(axis=0), f)
    zero = f == 0
    plus = ((per == 0) & ~np.signbit(per)).any(axis=0)                       # some tet gives +0.0 here
    minus_only = zero & np.signbit(f) & ~plus                                # the winner is -0.0 whatever the order of the tets
    ties = (((per == f[None]) & np.isfinite(per)).sum(axis=0) >= 2)
    positive = f > 0
    lo, h = -0.5, 1.0
    on_integer = sum(1 for tet in elem if all(((tet_v[tet, ax].astype(np.float64).min() - lo) / h - 0.5) % 1.0 == 0 for ax in range(3)))
    print(f"{name}: tets {len(elem)} zeros {int(zero.sum())} of them -0.0 with no +0.0 beside it {int(minus_only.sum())} ties {int(ties.sum())} "
          f"positive {int(positive.sum())} uncovered {int(np.isinf(f).sum())} tets with box limits on integers {on_integer}")
    assert on_integer == len(elem)
    # 400 random tets leave few nodes where -0.0 wins with no +0.0 beside it (somebody's face or interior covers most nodes): the sparse set
    # is there for those, the dense one for the ties
    want = {"kuhn2": dict(zeros=100, ties=100), "kuhn4": dict(zeros=100, ties=100, positive=1), "random": dict(zeros=100, ties=100, minus=1, positive=1),
            "sparse": dict(zeros=100, minus=5, positive=1)}[name]
    assert int(zero.sum()) >= want["zeros"] and int(ties.sum()) >= want.get("ties", 0)
    assert int(positive.sum()) >= want.get("positive", 0) and int(minus_only.sum()) >= want.get("minus", 0)
    out = U.union_field(tet_v, elem, G, _lattice_bounds(G))
    assert not np.signbit(out[zero]).any() and out.tobytes() == _lattice_field(name, G).tobytes()


@pytest.mark.parametrize("name", sorted(LATTICE))
def test_edge_lattice_boxes_meet_the_slab_seams(name):
    G = 48
    tet_v, elem = _lattice_tets(name, G)
    firsts, lasts = set(), set()
    for tet in elem:
        (i0, i1), _, _ = U.tet_box(tet_v[tet].astype(np.float64), G, -0.5, 1.0)
        firsts.add(i0)
        lasts.add(i1)
    print(f"{name}: tets {len(elem)} first planes {sorted(firsts)} last planes {sorted(lasts)}")
    assert SEAM_PLANES <= firsts and SEAM_PLANES <= lasts
    f = _lattice_field(name, G)
    assert (f == 0).sum() >= 100 and not np.signbit(f[f == 0]).any()


def test_edge_lattice_extraction_is_reached():
    """The lattice field at level exactly 0: the nodes that read 0 are outside, an edge from an inside node to one of them gets t = 1, and
    the triangles that meet there are degenerate.  At the default level they are inside."""
    G = 48
    f = _lattice_field("kuhn4", G)
    zeros = f == 0
    level = U.default_level(G, _lattice_bounds(G))
    assert zeros.sum() >= 100 and not U.occupancy(f, 0.0)[zeros].any() and U.occupancy(f, level)[zeros].all() and G ** 3 > 100 * 256
    v, faces, _ = U.extract_surface(f, _lattice_bounds(G), 0.0)
    p = v[faces].astype(np.float64)
    flat = int((np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1) == 0).sum())
    v1, faces1, _ = U.extract_surface(f, _lattice_bounds(G), level)
    print(f"zeros {int(zeros.sum())} level 0: triangles {len(faces)} degenerate {flat}; default level: triangles {len(faces1)}")
    assert flat > 0 and len(faces1) > 0


@gpu
@pytest.mark.parametrize("G", [8, 48])
@pytest.mark.parametrize("name", sorted(LATTICE))
def test_edge_lattice_tets(name, G):
    _field_both(*_lattice_tets(name, G), G, _lattice_bounds(G), want=_lattice_field(name, G))


@gpu
def test_edge_lattice_tets_wave_tail():
    """1 .. 9 tets: the last block of four waves holds 1, 2, 3 or 4 of them."""
    tet_v, elem = _lattice_tets("kuhn2", 8)
    for n in range(1, 10):
        _field_both(tet_v, elem[:n], 8, _lattice_bounds(8))


@gpu
def test_edge_extraction_at_many_workgroups():
    v, faces, closed = _extract_both(_random_field(33, 0, False), 0.0)
    assert not closed and len(faces) > 10000
    G = 48
    f = _lattice_field("kuhn4", G)
    _extract_both(f, float(U.default_level(G, _lattice_bounds(G))), _lattice_bounds(G))
    _extract_both(f, 0.0, _lattice_bounds(G))
