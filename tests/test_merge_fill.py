"""The merge's flood fill (tssplat_amd/merge.py: components, fill_field, merge_tets(fill=)): connected components of the field's
nodes under the extraction's own connectivity, enclosed cavities filled, islands dropped.  Everything is integers and bits: the
device results are compared with tests/fill_oracle.py bit for bit, and the oracle itself is checked on the CPU against
scipy.ndimage.label, the tree identity between node components and surface components, and the sub-mesh property."""
import functools
import inspect
import itertools
import os
import sys

import numpy as np
import pytest
import torch

import fill_oracle as F
import union_oracle as U
from tssplat_amd import _build, _capi, scenes

gpu = pytest.mark.gpu
INVALID = 1     # TSAMD_ERR_INVALID_ARGUMENT
UNIT = (-1.0, 1.0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------- fields and scenes ----------------------------------------------------------------
def _random_field(G, seed, border_outside=True):
    f = np.random.default_rng(1000 * seed + G).standard_normal((G, G, G)).astype(np.float32)
    if border_outside:
        f[0], f[-1], f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1] = -1, -1, -1, -1, -1, -1
    return f


CLOSED_CASES = [(9, 0.0), (12, -0.9), (17, -1.0)]              # (G, level): random fields with the border set to -1
SEEDS = (0, 1, 2)


def _special_field():
    """Values equal to the level, NaNs and infinities: the construction of test_merge.py's extraction test.  (field, level)"""
    G, level = 9, 0.25
    rng = np.random.default_rng(3)
    f = (np.round(rng.standard_normal((G, G, G)) * 4) / 4).astype(np.float32)
    assert (f == level).sum() > 20
    special = rng.permutation(G ** 3)[:60]
    f.reshape(-1)[special[:20]] = np.nan
    f.reshape(-1)[special[20:40]] = np.inf
    f.reshape(-1)[special[40:]] = -np.inf
    return f, level


@functools.lru_cache(maxsize=None)
def _shell_scene():
    """A hollow ball with a small ball floating in its void and a small ball far away: (tet_v float32, elem int32)."""
    bv, bt = scenes.kuhn_ball(6)
    bv = bv / np.linalg.norm(bv, axis=1).max()
    bt = bt[np.linalg.norm(bv[bt].mean(1), axis=1) >= 0.5]
    used, inverse = np.unique(bt, return_inverse=True)                  # drop the vertices of the removed core
    sv, st = bv[used], inverse.reshape(-1, 4)
    cv, ct = scenes.kuhn_ball(2)
    cv = cv / np.linalg.norm(cv, axis=1).max()
    centre = np.array([0.05, -0.02, 0.03])
    parts = [(sv * 0.7 + centre, st), (cv * 0.12 + centre, ct), (cv * 0.1 + np.array([0.85, 0.8, -0.8]), ct)]
    vs, ts, base = [], [], 0
    for v, t in parts:
        vs.append(v)
        ts.append(t + base)
        base += v.shape[0]
    return np.concatenate(vs).astype(np.float32), np.concatenate(ts).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _shell_merged(fill, grid=24, bounds=UNIT):
    v, e = _shell_scene()
    return F.merge_tets(v, e, grid, bounds, None, fill)


def _chi(m):
    return U.euler_characteristic(len(m["v"]), m["faces"])


def _serpentine_field(G):
    """One inside corridor, one node wide, through the whole grid, built by walking: it visits the planes i = 0, 2, 4, ..; in a plane
    the rows j = 0, 2, .. (or back); a row runs along k.  The joints are single nodes at the end the walk has reached.
    Returns (field, path length)."""
    f = np.full((G, G, G), -1, np.float32)
    k_end, j_dir, j = G - 1, 1, 0
    length = 0
    for i in range(0, G, 2):
        rows = list(range(0, G, 2))
        if j_dir < 0:
            rows.reverse()
        for n, j in enumerate(rows):
            f[i, j, :] = 1
            length += G
            if n + 1 < len(rows):
                f[i, j + j_dir, k_end] = 1                              # the joint to the next row, at the end the walk has reached
                length += 1
                k_end = G - 1 - k_end
        if i + 2 < G:
            f[i + 1, j, k_end] = 1                                      # the joint to the next plane
            length += 1
            k_end = G - 1 - k_end
            j_dir = -j_dir
    return f, length


def _slabs(G, at):
    """Two inside slabs, i <= at - 2 and i >= at + 3 (empty when the grid ends first), each with a pillar towards the other; the pillars
    touch only through the (1, 1, 1) edge (at, at, at) - (at + 1, at + 1, at + 1)."""
    f = np.full((G, G, G), -1, np.float32)
    f[:at - 1] = 1
    f[at + 3:] = 1
    f[at - 1:at + 1, at, at] = 1                                          # a pillar from the lower slab up to (at, at, at)
    f[at + 1:at + 3, at + 1, at + 1] = 1                                  # and one from (at + 1, at + 1, at + 1) up to the upper slab
    return f


# ---------------------------------------------------------------- CPU: the oracle ----------------------------------------------------------------
def _same_partition(a, b):
    """Two labellings of the same nodes induce the same partition."""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    pairs = np.unique(np.stack([a, b], 1), axis=0)
    return len(pairs) == len(np.unique(a)) == len(np.unique(b))


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("G,level", CLOSED_CASES)
def test_oracle_components_equal_scipy_label(G, level, seed):
    ndimage = pytest.importorskip("scipy").ndimage
    structure = np.zeros((3, 3, 3), dtype=bool)
    structure[1, 1, 1] = True
    for di, dj, dk in F.OWNED:
        structure[1 + di, 1 + dj, 1 + dk] = structure[1 - di, 1 - dj, 1 - dk] = True
    assert structure.sum() == 15 and not structure[2, 0, 1] and not structure[1, 2, 0]          # 14 neighbours; (1, -1, 0) is no edge
    f = _random_field(G, seed)
    inside = U.occupancy(f, level)
    label = F.components(f, level)
    assert label.dtype == np.int32 and label.shape == (G, G, G)
    flat = label.reshape(-1)
    assert (flat <= np.arange(G ** 3)).all() and np.array_equal(flat[flat], flat)
    assert np.array_equal(inside.reshape(-1)[flat], inside.reshape(-1))                          # a component has one inside bit
    for mask in (inside, ~inside):
        want, count = ndimage.label(mask, structure=structure)
        assert count == len(np.unique(label[mask])) and _same_partition(label[mask], want[mask])
        for lab in np.unique(label[mask]):                                                       # the label is the component's minimum
            assert lab == np.flatnonzero(label.reshape(-1) == lab).min()
    n_out = len(np.unique(label[~inside]))
    assert n_out >= (2 if G > 9 else 1)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("G,level", CLOSED_CASES)
def test_oracle_surface_components_are_node_components_minus_one(G, level, seed):
    """The tree identity: every surface separates one inside from one outside component, and the adjacency graph is a tree."""
    f = _random_field(G, seed)
    v, faces, closed = U.extract_surface(f, UNIT, level)
    assert closed and U.edge_defects(faces) == 0
    label, inside = F.components(f, level), U.occupancy(f, level)
    assert F.count_mesh_components(len(v), faces) == len(np.unique(label[inside])) + len(np.unique(label[~inside])) - 1


@pytest.mark.parametrize("seed", SEEDS[:2])
@pytest.mark.parametrize("G,level", CLOSED_CASES)
def test_oracle_filled_extraction_is_a_submesh(G, level, seed):
    f = _random_field(G, seed)
    v, faces, _ = U.extract_surface(f, UNIT, level)
    inside = U.occupancy(f, level)
    n_surfaces = F.count_mesh_components(len(v), faces)
    solid = U.occupancy(F.fill_field(f, level, "cavities")["field"], level)
    for mode in F.MODES:
        r = F.fill_field(f, level, mode)
        g = r["field"]
        after = U.occupancy(g, level)
        same = after == inside
        assert g[same].tobytes() == f[same].tobytes() and (g[after & ~inside] == np.inf).all() and (g[~after & inside] == -np.inf).all()
        assert r["cavity_nodes"] == int((solid & ~inside).sum()) and not (inside & ~solid).any()
        gv, gf, closed = U.extract_surface(g, UNIT, level)
        assert closed and U.edge_defects(gf) == 0
        assert F.submesh_of(gv, gf, v, faces)
        label = F.components(g, level)
        assert len(np.unique(label[~after])) == 1                                                # one outside component: the exterior
        surfaces = F.count_mesh_components(len(gv), gf)
        if mode == "cavities":
            assert r["islands"] == r["island_nodes"] == 0 and surfaces == len(np.unique(label[after]))
            n_outside = len(np.unique(F.components(f, level)[~inside]))
            assert n_surfaces - surfaces >= r["cavities"] == n_outside - 1                        # each cavity's surface and those of the islands in it
        else:
            assert surfaces == 1 and len(np.unique(label[after])) == 1 and r["island_nodes"] >= r["islands"]
            assert not (after & ~solid).any() and int(after.sum()) == int(solid.sum()) - r["island_nodes"]


def test_oracle_shell_scene_has_a_void_an_island_in_it_and_an_island_outside():
    none, cav, outer = (_shell_merged(fill) for fill in ("none", "cavities", "outer"))
    inside = U.occupancy(none["field"], none["level"])
    label = F.components(none["field"], none["level"])
    assert len(np.unique(label[inside])) == 3 and len(np.unique(label[~inside])) == 2
    assert [F.count_mesh_components(len(m["v"]), m["faces"]) for m in (none, cav, outer)] == [4, 2, 1]
    assert [_chi(m) for m in (none, cav, outer)] == [8, 4, 2]
    for m in (none, cav, outer):
        assert m["closed"] and U.edge_defects(m["faces"]) == 0
    in_cav, in_outer = U.occupancy(cav["field"], cav["level"]), U.occupancy(outer["field"], outer["level"])
    assert int((in_cav & ~inside).sum()) == 315 and not (inside & ~in_cav).any()
    assert int((in_cav & ~in_outer).sum()) == 2 and not (in_outer & ~in_cav).any()
    assert (cav["cavities"], cav["cavity_nodes"], cav["islands"], cav["island_nodes"]) == (1, 315, 0, 0)
    assert (outer["cavities"], outer["cavity_nodes"], outer["islands"], outer["island_nodes"]) == (1, 315, 1, 2)
    assert none["fill"] == "none" and cav["fill"] == "cavities" and outer["inside_fraction"] == in_outer.sum() / 24 ** 3
    for m in (cav, outer):
        assert F.submesh_of(m["v"], m["faces"], none["v"], none["faces"])
    plain = U.merge_tets(*_shell_scene(), 24, UNIT)
    assert plain["v"].tobytes() == none["v"].tobytes() and plain["faces"].tobytes() == none["faces"].tobytes()


def test_oracle_chains_and_serpentine():
    G = 9
    f, length = _serpentine_field(G)
    inside = f > 0
    label = F.components(f, 0.0)
    assert int(inside.sum()) == length >= G ** 3 // 4 and len(np.unique(label[inside])) == 1
    # remove one joint: two components, so the corridor really is one node wide
    g = f.copy()
    g[1, G - 1, :] = -1
    assert len(np.unique(F.components(g, 0.0)[g > 0])) == 2
    body, anti = np.full((G, G, G), -1, np.float32), np.full((G, G, G), -1, np.float32)
    idx = np.arange(G)
    body[idx, idx, idx] = 1
    anti[idx, G - 1 - idx, 0] = 1
    assert len(np.unique(F.components(body, 0.0)[body > 0])) == 1 and len(np.unique(F.components(anti, 0.0)[anti > 0])) == G
    s = _slabs(G, 4)
    assert len(np.unique(F.components(s, 0.0)[s > 0])) == 1
    s[4, 4, 4] = -1
    assert len(np.unique(F.components(s, 0.0)[s > 0])) == 2


# ---------------------------------------------------------------- CPU: argument checks ----------------------------------------------------------------
def test_c_abi_argument_errors_launch_nothing():
    """Every argument error is reported before anything touches the device: all device pointers here are null or made up."""
    lib = _capi.load()
    p, q = 0x1000, 0x2000                                                 # "not null"; never dereferenced on these paths

    def comps(f=p, grid=8, level=0.0, label=p, status=p):
        return lib.tsamd_grid_components(f, grid, level, label, status, None)

    def fill(f=p, grid=8, level=0.0, mode=1, work=p, out=q, stats=p):
        return lib.tsamd_field_fill(f, grid, level, mode, work, out, stats, None)

    nan = float("nan")
    cases = [
        (comps, dict(grid=1), "grid"), (comps, dict(grid=513), "grid"), (comps, dict(grid=-4), "grid"), (comps, dict(level=nan), "level"),
        (comps, dict(f=None), "field_dev"), (comps, dict(label=None), "label_out_dev"), (comps, dict(status=None), "status_out_dev"),
        (fill, dict(grid=1), "grid"), (fill, dict(grid=513), "grid"), (fill, dict(level=nan), "level"), (fill, dict(mode=0), "mode"),
        (fill, dict(mode=3), "mode"), (fill, dict(mode=-1), "mode"), (fill, dict(f=None), "field_dev"), (fill, dict(work=None), "workspace_dev"),
        (fill, dict(out=None), "field_out_dev"), (fill, dict(stats=None), "stats_out_dev"), (fill, dict(out=p), "field_out_dev"),
        (fill, dict(work=0x1004), "workspace_dev"),
    ]
    for fn, kw, word in cases:
        assert fn(**kw) == INVALID, (fn.__name__, kw)
        msg = lib.tsamd_last_error().decode()
        assert msg and word in msg, (fn.__name__, kw, msg)
    assert _capi.ABI_VERSION == 3 and lib.tsamd_abi_version() == 3        # nothing existing changed


def test_python_arguments_are_checked_by_name():
    """Nothing here reaches the library: a CPU tensor or a bad mode is refused first, with the argument's name."""
    from tssplat_amd import merge
    v, e, f = torch.zeros(4, 3), torch.zeros(1, 4, dtype=torch.int32), torch.zeros(4, 4, 4)
    for call, word in [(lambda: merge.components(f, 0.0), "field"), (lambda: merge.components(np.zeros((4, 4, 4), np.float32), 0.0), "field"),
                       (lambda: merge.fill_field(f, 0.0, "cavities"), "field"), (lambda: merge.merge_tets(v, e, fill="both"), "fill must be one of"),
                       (lambda: merge.merge_tets(v, e, fill=None), "fill must be one of"), (lambda: merge.merge_tets(v, e, fill="outer"), "tet_v")]:
        with pytest.raises(RuntimeError, match=word):
            call()
    assert merge.FILL_MODES == {"cavities": 1, "outer": 2}
    with pytest.raises(RuntimeError, match="mode must be one of"):
        merge._check_fill("fill_field", "none", allow_none=False)
    with pytest.raises(RuntimeError, match="level"):
        merge._check_level("components", float("nan"))


def test_build_lists_carry_the_fill_source():
    assert "fill_kernels.hip" in _build.SOURCES and "merge.h" in _build.HEADERS
    assert "fill_kernels.hip" not in _build.SOURCE_FLAGS                  # integers only: no contraction flag
    assert os.path.exists(os.path.join(_build.CSRC, "fill_kernels.hip"))
    assert {"tsamd_grid_components", "tsamd_field_fill"} <= set(_capi.SIGNATURES)


def test_fill_none_is_the_default_everywhere():
    from tssplat_amd import geometry, merge, renderers
    for fn in (merge.merge_tets, geometry.TetMeshGeometry.export_merged, renderers.MeshRasterizer.export_merged):
        assert inspect.signature(fn).parameters["fill"].default == "none", fn
    fields = {f.name: f.default for f in __import__("dataclasses").fields(merge.MergedSurface)}
    assert (fields["fill"], fields["cavities"], fields["cavity_nodes"], fields["islands"], fields["island_nodes"]) == ("none", 0, 0, 0, 0)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import train_object
    finally:
        sys.path.pop(0)
    assert inspect.signature(train_object.run).parameters["merge_fill"].default == "none"
    assert F.merge_tets.__defaults__[-1] == "none"


# ---------------------------------------------------------------- GPU: the labels ----------------------------------------------------------------
def _labels_both(f, level):
    from tssplat_amd import merge
    want = F.components(f, level)
    got = merge.components(dev(f), level)
    assert got.dtype == torch.int32 and tuple(got.shape) == f.shape
    # the invariants, on the device result itself
    flat = got.reshape(-1).long()
    assert bool((flat <= torch.arange(flat.numel(), device=flat.device)).all()) and bool((flat[flat] == flat).all())
    got = got.cpu().numpy()
    assert got.tobytes() == want.tobytes(), int((got != want).sum())
    return want


@gpu
@pytest.mark.parametrize("border_outside", [True, False])
@pytest.mark.parametrize("G", [2, 5, 9, 12])
def test_labels_of_random_fields_equal_oracle(G, border_outside):
    for level in (0.0, -0.9):
        _labels_both(_random_field(G, 0, border_outside), level)


@gpu
def test_labels_with_exact_level_values_nans_and_infinities():
    f, level = _special_field()
    _labels_both(f, level)
    _labels_both(f, float("inf"))                                         # nothing is inside
    _labels_both(f, float("-inf"))


@gpu
@pytest.mark.parametrize("G", [2, 5])
def test_labels_of_constant_fields_and_one_corner_node(G):
    for value in (-1, 1):
        want = _labels_both(np.full((G, G, G), value, np.float32), 0.0)
        assert not want.any()                                             # one component: label 0 everywhere
    for corner in [(0, 0, 0), (G - 1, G - 1, G - 1), (0, G - 1, 0)]:
        f = np.full((G, G, G), -1, np.float32)
        f[corner] = 1
        want = _labels_both(f, 0.0)
        assert len(np.unique(want)) == 2


@gpu
def test_labels_of_a_serpentine_corridor():
    G = 33
    f, length = _serpentine_field(G)
    assert length >= G ** 3 // 4
    want = _labels_both(f, 0.0)
    assert len(np.unique(want[f > 0])) == 1


@gpu
def test_labels_of_diagonal_chains():
    G = 33
    idx = np.arange(G)
    body, anti = np.full((G, G, G), -1, np.float32), np.full((G, G, G), -1, np.float32)
    body[idx, idx, idx] = 1
    anti[idx, G - 1 - idx, 0] = 1
    assert len(np.unique(_labels_both(body, 0.0)[body > 0])) == 1
    assert len(np.unique(_labels_both(anti, 0.0)[anti > 0])) == G


@gpu
@pytest.mark.parametrize("at", [15, 31])
def test_labels_of_slabs_joined_by_one_body_diagonal(at):
    f = _slabs(33, at)
    assert f[at, at, at] > 0 and f[at + 1, at + 1, at + 1] > 0
    assert len(np.unique(_labels_both(f, 0.0)[f > 0])) == 1
    f[at, at, at] = -1
    assert len(np.unique(_labels_both(f, 0.0)[f > 0])) == 2


@gpu
def test_labels_at_grid_65_and_repeatable():
    from tssplat_amd import merge
    f = _random_field(65, 0)
    _labels_both(f, 0.0)
    a = merge.components(dev(f), 0.0).cpu().numpy()
    b = merge.components(dev(f), 0.0).cpu().numpy()
    assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- GPU: the fill ----------------------------------------------------------------
def _extract_bytes(field, level, bounds=UNIT):
    from tssplat_amd import merge
    v, faces, closed = merge.extract_surface(field, bounds, level)
    return v.cpu().numpy(), faces.cpu().numpy(), closed


def _fill_both(f, level, mode):
    from tssplat_amd import merge
    want = F.fill_field(f, level, mode)
    src = dev(f)
    got = merge.fill_field(src, level, mode)
    assert isinstance(got, merge.FilledField) and got.field.dtype == torch.float32 and got.field.data_ptr() != src.data_ptr()
    assert src.cpu().numpy().tobytes() == f.tobytes()                     # the input is unchanged
    assert got.field.cpu().numpy().tobytes() == want["field"].tobytes()
    assert (got.cavities, got.cavity_nodes, got.islands, got.island_nodes) == tuple(want[k] for k in ("cavities", "cavity_nodes", "islands", "island_nodes"))
    assert all(isinstance(x, int) for x in (got.cavities, got.cavity_nodes, got.islands, got.island_nodes))
    wv, wf, wc = U.extract_surface(want["field"], UNIT, level)
    v, faces, closed = _extract_bytes(got.field, level)
    assert v.tobytes() == wv.tobytes() and faces.tobytes() == wf.tobytes() and closed == wc
    return want, (v, faces)


@gpu
@pytest.mark.parametrize("mode", F.MODES)
@pytest.mark.parametrize("G,level", CLOSED_CASES)
def test_fill_of_random_fields_equals_oracle_and_is_a_submesh(G, level, mode):
    f = _random_field(G, 0)
    want, (v, faces) = _fill_both(f, level, mode)
    v0, f0, _ = _extract_bytes(dev(f), level)                               # the sub-mesh property, on device results
    assert F.submesh_of(v, faces, v0, f0)
    if G > 9:                                                             # (the G = 9 field may have nothing to fill)
        assert want["cavities"] > 0 and len(faces) < len(f0)
    if mode == "outer":
        assert F.count_mesh_components(len(v), faces) == 1 and U.edge_defects(faces) == 0


@gpu
@pytest.mark.parametrize("mode", F.MODES)
def test_fill_with_special_values_and_of_the_shell_scene(mode):
    f, level = _special_field()
    f[0], f[-1], f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1] = -1, -1, -1, -1, -1, -1
    _fill_both(f, level, mode)
    none = _shell_merged("none")
    want, _ = _fill_both(none["field"], none["level"], mode)
    assert want["cavity_nodes"] == 315 and want["island_nodes"] == (2 if mode == "outer" else 0)


@gpu
@pytest.mark.parametrize("mode", F.MODES)
def test_fill_of_a_grid_that_is_not_closed(mode):
    """Inside nodes on the border: nothing special about them -- only outside border nodes make an exterior."""
    for G in (5, 12):
        want, _ = _fill_both(_random_field(G, 1, border_outside=False), 0.0, mode)
    _fill_both(np.full((5, 5, 5), 1, np.float32), 0.0, mode)               # all inside: no exterior at all
    _fill_both(np.full((2, 2, 2), -1, np.float32), 0.0, mode)              # all outside: no solid at all
    f = np.full((5, 5, 5), 1, np.float32)
    f[2, 2, 2] = -1                                                       # one enclosed node in a solid block that reaches the border
    want, _ = _fill_both(f, 0.0, mode)
    assert want["cavities"] == want["cavity_nodes"] == 1


@gpu
def test_outer_tie_goes_to_the_smaller_label():
    f = np.full((9, 9, 9), -1, np.float32)
    f[5:7, 5:7, 5:7] = 1
    f[1:3, 1:3, 1:3] = 1
    want, _ = _fill_both(f, 0.0, "outer")
    assert want["islands"] == 1 and want["island_nodes"] == 8 and want["field"][1, 1, 1] == 1 and want["field"][5, 5, 5] == -np.inf


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
@pytest.mark.parametrize("fill", ["none", "cavities", "outer"])
def test_merge_tets_with_fill_equals_oracle(fill):
    from tssplat_amd import merge
    v, e = _shell_scene()
    want = _shell_merged(fill)
    got = merge.merge_tets(dev(v), dev(e), grid=24, bounds=UNIT, fill=fill) if fill != "none" else merge.merge_tets(dev(v), dev(e), grid=24, bounds=UNIT)
    assert got.fill == fill and got.grid == 24 and got.bounds == want["bounds"] and got.level == want["level"]
    assert got.closed is True and want["closed"] and got.inside_fraction == want["inside_fraction"]
    assert (got.cavities, got.cavity_nodes, got.islands, got.island_nodes) == tuple(want[k] for k in ("cavities", "cavity_nodes", "islands", "island_nodes"))
    assert got.v.cpu().numpy().tobytes() == want["v"].tobytes() and got.faces.cpu().numpy().tobytes() == want["faces"].tobytes()
    if fill == "none":
        plain = U.merge_tets(v, e, 24, UNIT)
        assert got.v.cpu().numpy().tobytes() == plain["v"].tobytes() and got.faces.cpu().numpy().tobytes() == plain["faces"].tobytes()
        assert got.inside_fraction == plain["inside_fraction"]


@gpu
def test_geometry_export_merged_outer_writes_that_mesh(tmp_path):
    from tssplat_amd import geometry
    v, e = _shell_scene()
    geo = geometry.TetMeshGeometry(v, e, use_smooth_barrier=False)
    merged = geo.export_merged(str(tmp_path / "out"), "final", grid=24, bounds=UNIT, fill="outer")
    want = _shell_merged("outer")
    rv, rf = _read_plain_obj(tmp_path / "out" / "final_merged.obj")
    assert merged.fill == "outer" and (merged.cavities, merged.islands) == (1, 1)
    assert rv.tobytes() == want["v"].tobytes() == merged.v.cpu().numpy().tobytes()
    assert rf.tobytes() == want["faces"].tobytes() == merged.faces.cpu().numpy().tobytes()


@gpu
def test_renderer_export_merged_outer_writes_that_mesh(tmp_path):
    from tssplat_amd import atlas, geometry, renderers

    class Field(torch.nn.Module):
        def forward(self, positions):
            return {"color": 0.5 + 0.5 * torch.sin(torch.stack([3.0 * positions[..., 0] + 1.0, 4.0 * positions[..., 1], 5.0 * positions[..., 2] - 0.5], -1))}

    v, e = _shell_scene()
    geo = geometry.TetMeshGeometry(v, e, use_smooth_barrier=False, optimize_geo=False)
    merged = renderers.MeshRasterizer(geo, Field()).export_merged(str(tmp_path), "material", grid=24, fill="outer")
    want = _shell_merged("outer", 24, None)                               # the renderer's export takes the default bounds
    assert want["cavities"] + want["islands"] > 0 and merged.fill == "outer"
    assert (merged.cavities, merged.cavity_nodes, merged.islands, merged.island_nodes) == tuple(want[k] for k in ("cavities", "cavity_nodes", "islands", "island_nodes"))
    rv, rf, _, _, _ = atlas.load_textured_obj(str(tmp_path / "material"), "merged_surface")
    assert rv.tobytes() == want["v"].tobytes() and rf.tobytes() == want["faces"].tobytes()
    assert F.count_mesh_components(len(rv), rf) == 1


# ---------------------------------------------------------------- edges: every neighbourhood on every tile seam ----------------------------------------------------------------
# Which owned edges the kernels unite depends on a node's neighbourhood (needed_edges prunes the implied ones) and on which faces of
# its 4 x 8 x 16 tile it sits on (the tile kernel takes the edges that stay inside, the merge kernel those that leave).  What decides is
# the node's own inside bit and whether each of ten neighbours shares it: the seven owned neighbours v + (di, dj, dk) and the three nodes
# one step back along k from v, v + (1, 0, 0) and v + (0, 1, 0) -- an 11-bit pattern -- and the three booleans "on the tile's upper i / j / k
# face" -- 8 classes.  Random fields alone leave thousands of the 16 384 combinations out, most of them on the tile's corner nodes
# (315 per 64-grid) and its j-k edge; here the rare classes get their patterns planted.
TILE = (4, 8, 16)
SEAM_G, SEAM_FIELDS = 64, 7
BACK = ((0, 0), (1, 0), (0, 1))                                              # (di, dj) of the three nodes one step back along k


def _neighbourhood_codes(inside):
    """int32 [G - 1, G - 1, G - 2]: 8 pattern + class for every node (i, j, k) with i, j < G - 1 and 1 <= k < G - 1, the nodes whose ten
    neighbours all exist.  Pattern: bit 0 the inside bit, bit m (1 .. 7) "node + (m >> 2 & 1, m >> 1 & 1, m & 1) has the same bit", bits
    8, 9, 10 the same for the three BACK nodes.  Class: 4 top_i + 2 top_j + top_k."""
    G = inside.shape[0]
    own = inside[:G - 1, :G - 1, 1:G - 1]
    pattern = own.astype(np.int32)
    for m, (di, dj, dk) in enumerate(F.OWNED, start=1):
        pattern |= (inside[di:G - 1 + di, dj:G - 1 + dj, 1 + dk:G - 1 + dk] == own).astype(np.int32) << m
    for n, (di, dj) in enumerate(BACK):
        pattern |= (inside[di:G - 1 + di, dj:G - 1 + dj, 0:G - 2] == own).astype(np.int32) << (8 + n)
    i, j, k = np.meshgrid(np.arange(G - 1), np.arange(G - 1), np.arange(1, G - 1), indexing="ij")
    top = [(x & (t - 1)) == t - 1 for x, t in zip((i, j, k), TILE)]
    return pattern * 8 + (top[0] * 4 + top[1] * 2 + top[2])


def _plant(inside, node, pattern):
    """Give `node` the 11-bit pattern: writes its 2 x 2 x 3 footprint's twelve nodes but (i + 1, j + 1, k - 1)."""
    i, j, k = node
    own = bool(pattern & 1)
    inside[i, j, k] = own
    for m, (di, dj, dk) in enumerate(F.OWNED, start=1):
        inside[i + di, j + dj, k + dk] = own == bool((pattern >> m) & 1)
    for n, (di, dj) in enumerate(BACK):
        inside[i + di, j + dj, k - 1] = own == bool((pattern >> (8 + n)) & 1)


def _plant_sites(G, cls):
    """The nodes of class `cls` on a sub-lattice whose footprints are disjoint: i = 1 or 3 (top) mod 4, j = 1, 3, 5 or 7 (top) mod 8,
    k = 2, 5, 8, 11 or 15 (top) mod 16 -- the footprint i .. i + 1, j .. j + 1, k - 1 .. k + 1 of one site ends before the next one's begins."""
    def axis(top, tile, low, first=0):
        rest = (tile - 1,) if top else low
        return [x for x in range(first, G - 1) if x % tile in rest]
    return list(itertools.product(axis(cls & 4, 4, (1,)), axis(cls & 2, 8, (1, 3, 5)), axis(cls & 1, 16, (2, 5, 8, 11), 1)))


@functools.lru_cache(maxsize=None)
def _seam_fields():
    """SEAM_FIELDS boolean grids of SEAM_G^3 nodes, random at p = 0.5.  In field f the c-th site of the corner class (all three faces) and
    of the j-k edge class gets the pattern (sites per field x f + c) mod 2048, which runs through all 2048 in seven fields; whatever the
    count then still reports missing is planted on unused sites of its class, round by round (a plant can take a random neighbour's
    pattern away).  The coverage is asserted by test_edge_seam_fields_cover_every_neighbourhood, from the fields alone."""
    G = SEAM_G
    fields = [np.random.default_rng(4000 + f).random((G, G, G)) < 0.5 for f in range(SEAM_FIELDS)]
    used = [set() for _ in fields]
    for cls in (7, 3):
        sites = _plant_sites(G, cls)
        for f, inside in enumerate(fields):
            for c, node in enumerate(sites):
                _plant(inside, node, (len(sites) * f + c) % 2048)
                used[f].add(node)
    for _ in range(8):
        seen = np.zeros(16384, dtype=bool)
        for inside in fields:
            seen[np.unique(_neighbourhood_codes(inside))] = True
        missing = np.flatnonzero(~seen)
        if not missing.size:
            break
        for n, code in enumerate(missing.tolist()):
            f = n % SEAM_FIELDS
            node = next(s for s in _plant_sites(G, code & 7) if s not in used[f])
            _plant(fields[f], node, code >> 3)
            used[f].add(node)
    return tuple(fields)


def _as_field(inside, border_outside=False):
    f = np.where(inside, np.float32(1), np.float32(-1))
    if border_outside:
        f[0], f[-1], f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1] = -1, -1, -1, -1, -1, -1
    return f


def test_edge_seam_fields_cover_every_neighbourhood():
    counts = np.zeros(16384, dtype=np.int64)
    for inside in _seam_fields():
        counts += np.bincount(_neighbourhood_codes(inside).reshape(-1), minlength=16384)
    per_class = [(int((counts[c::8] > 0).sum()), int(counts[c::8].min())) for c in range(8)]
    print(f"covered {int((counts > 0).sum())} of 16384; per class (top_i top_j top_k as bits 4 2 1) patterns seen, fewest nodes on one pattern: {per_class}")
    assert (counts > 0).all()
    # the counting itself, on a case small enough to read: one inside node in an outside grid
    one = np.zeros((20, 20, 20), dtype=bool)
    one[3, 7, 15] = True
    codes = _neighbourhood_codes(one)                                        # indexed [i, j, k - 1]
    assert codes[3, 7, 14] == 8 * 1 + 7                                      # inside, nobody shares the bit; the corner class
    assert codes[2, 7, 14] == 8 * (0x7FE & ~(1 << 4)) + 3                    # its lower i neighbour: all share but node + (1, 0, 0); j-k edge class
    assert codes[3, 7, 15] == 8 * (0x7FE & ~(1 << 8)) + 6                    # the node after it along k: all but the one straight back; i-j edge class


def test_edge_random_fields_alone_leave_combinations_out():
    """Why the plants: seven random 64-grids without them."""
    seen = np.zeros(16384, dtype=bool)
    for f in range(SEAM_FIELDS):
        seen[np.unique(_neighbourhood_codes(np.random.default_rng(4000 + f).random((SEAM_G,) * 3) < 0.5))] = True
    print(f"random alone: {int(seen.sum())} of 16384; corner class {int(seen[7::8].sum())}, j-k edge class {int(seen[3::8].sum())} of 2048")
    assert seen[7::8].sum() < 2048 and seen[3::8].sum() < 2048


DENSITY_CASES = [(G, p) for G in (16, 17, 32) for p in (0.03, 0.5, 0.97)]
CONSTANT_CASES = [(G, value) for G in (16, 17, 33) for value in (1, -1)]


def _density_field(G, p, border_outside=False):
    return _as_field(np.random.default_rng(int(1000 * p) + G).random((G, G, G)) < p, border_outside)


@pytest.mark.parametrize("G,p", DENSITY_CASES)
def test_edge_grid_sizes_and_densities_are_reached(G, p):
    """16 and 32 are whole tiles on every axis (no lane beyond the grid); 17 adds one valid plane, row and column of otherwise empty tiles.
    At p = 0.03 the solid is dozens to hundreds of specks (about 0.03 (G - 2)^3 nodes, few of them adjacent), at 0.97 the outside is."""
    assert [G % t for t in TILE] == ([0, 0, 0] if G != 17 else [1, 1, 1])
    f = _density_field(G, p, border_outside=True)
    inside = f > 0
    label = F.components(f, 0.0)
    n_in, n_out = len(np.unique(label[inside])), len(np.unique(label[~inside]))
    r = F.fill_field(f, 0.0, "outer")
    print(f"G {G} p {p}: inside {inside.mean():.3f} components inside {n_in} outside {n_out} cavities {r['cavities']} islands {r['islands']}")
    if p == 0.03:
        assert n_in > 20 and r["islands"] > 20
    if p == 0.97:
        assert n_out > 20 and r["cavities"] > 20


def test_edge_many_equal_components_are_reached():
    G = 33
    f = np.full((G, G, G), -1, np.float32)
    f[1:-1:2, 1:-1:2, 1:-1:2] = 1
    label = F.components(f, 0.0)
    labs, counts = np.unique(label[f > 0], return_counts=True)
    assert len(labs) == 4096 and (counts == 1).all()                         # no two odd nodes are Kuhn-adjacent
    r = F.fill_field(f, 0.0, "outer")
    assert (r["cavities"], r["cavity_nodes"], r["islands"], r["island_nodes"]) == (0, 0, 4095, 4095)
    assert r["field"][1, 1, 1] == 1 and int((r["field"] > 0).sum()) == 1     # the smallest label stays
    g = _as_field(~(f > 0), border_outside=True)
    r = F.fill_field(g, 0.0, "cavities")
    print(f"solid components {len(labs)}; inverse field: cavities {r['cavities']} cavity nodes {r['cavity_nodes']}")
    assert (r["cavities"], r["cavity_nodes"], r["islands"], r["island_nodes"]) == (2744, 2744, 0, 0)


@gpu
@pytest.mark.parametrize("f", range(SEAM_FIELDS))
def test_edge_seam_fields_labels(f):
    _labels_both(_as_field(_seam_fields()[f]), 0.0)


@gpu
@pytest.mark.parametrize("mode", F.MODES)
@pytest.mark.parametrize("f", [0, SEAM_FIELDS - 1])
def test_edge_seam_fields_fill(f, mode):
    want, _ = _fill_both(_as_field(_seam_fields()[f], border_outside=True), 0.0, mode)
    assert want["cavities"] > 0


@gpu
@pytest.mark.parametrize("G,p", DENSITY_CASES)
def test_edge_grid_sizes_and_densities(G, p):
    _labels_both(_density_field(G, p), 0.0)
    _labels_both(_density_field(G, p, border_outside=True), 0.0)
    if p != 0.5:
        for mode in F.MODES:
            _fill_both(_density_field(G, p, border_outside=True), 0.0, mode)
            _fill_both(_density_field(G, p), 0.0, mode)


@gpu
@pytest.mark.parametrize("G,value", CONSTANT_CASES)
def test_edge_constant_fields_over_many_tiles(G, value):
    want = _labels_both(np.full((G, G, G), value, np.float32), 0.0)
    assert not want.any()                                                    # one component: label 0 everywhere


@gpu
@pytest.mark.parametrize("mode", F.MODES)
def test_edge_many_equal_components(mode):
    G = 33
    f = np.full((G, G, G), -1, np.float32)
    f[1:-1:2, 1:-1:2, 1:-1:2] = 1
    want, _ = _fill_both(f, 0.0, mode)
    assert want["islands"] == (4095 if mode == "outer" else 0)
    want, _ = _fill_both(_as_field(~(f > 0), border_outside=True), 0.0, mode)
    assert want["cavities"] == want["cavity_nodes"] == 2744
