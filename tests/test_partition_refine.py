"""CPU tests of the refined partition (tssplat_amd/csrc/partition.cpp: cells grown over the face adjacency, Fiduccia-Mattheyses
passes, the cut of a template shared by its copies).  Plans are built with ``host_only=True`` and ``max_threads=768`` -- an
explicit tiling option keeps the fullest tiles that fit, the path the partitioner serves.  No compute kernel runs here."""
import numpy as np
import pytest

from oracle import tet_energy_oracle as O
from tssplat_amd import scenes
import tile_emulator as TE

# slots + staged rows of the same three plans at commit c37ac6b (greedy strictly-improving moves, cost 3 * slots + tile vertices),
# read from plan_info() there: total_slots + shared_vertex_copies
PARENT = {"kuhn8": 3729 + 848, "kuhn10": 7539 + 1967, "aveg": 26675 + 5610}
KW = {"kuhn8": dict(lds_budget_bytes=40000), "kuhn10": dict(lds_budget_bytes=40000), "aveg": {}}
LDS = {"kuhn8": 40000, "kuhn10": 40000, "aveg": 81920}


def _plan(sc, **kw):
    from tssplat_amd import tet_spheres_ext as ext
    return ext.TetSpheres(sc.rest.reshape(-1), sc.tets.reshape(-1), host_only=True, **{"max_threads": 768, **kw})


@pytest.fixture(scope="module")
def inputs(aveg):
    rest, tets = aveg
    return {"kuhn8": scenes.make_scene("kuhn8", 1), "kuhn10": scenes.make_scene("kuhn10", 1),
            "aveg": scenes.replicate_spheres(rest.astype(np.float64), tets, 1, seed=3)}


@pytest.fixture(scope="module")
def plans(inputs):
    return {name: _plan(sc, **KW[name]) for name, sc in inputs.items()}


def _owned(T, spt):
    slot = np.arange(T["s_pad"])
    item = (slot % spt) * (T["s_pad"] // spt) + slot // spt
    return T["slot_tet"][(item < T["n_owned"]) & (T["slot_tet"] >= 0)]


def _face_connected(tets, nbr):
    inside = np.zeros(nbr.shape[0], bool)
    inside[tets] = True
    seen = np.zeros_like(inside)
    seen[tets[0]] = True
    front = np.array([tets[0]])
    while front.size:
        q = nbr[front].ravel()
        q = q[q >= 0]
        q = np.unique(q[inside[q] & ~seen[q]])
        seen[q] = True
        front = q
    return int(seen.sum()) == tets.size


def _cells(ts):
    spt = ts.plan_info()["slots_per_thread"]
    return [np.sort(_owned(T, spt)) for T in TE.plan_tiles(ts)]


def _plan_bytes(ts):
    out = []
    for T in TE.plan_tiles(ts):
        out += [T[k].tobytes() for k in ("planes", "gvid", "vdst", "slot_tet", "row_start")]
    return b"".join(out)


@pytest.mark.parametrize("name", ["kuhn8", "kuhn10", "aveg"])
def test_every_tet_is_owned_once_and_every_cell_is_connected_and_fits(name, inputs, plans):
    sc, ts = inputs[name], plans[name]
    info = ts.plan_info()
    assert info["n_tiles"] >= 4 and info["cut_components"] == 1
    assert info["owned_tets"] == sc.n_tets and info["halo_slots"] == info["total_slots"] - sc.n_tets
    assert info["staged_rows"] == info["shared_vertex_copies"] and info["min_tiles"] <= info["n_tiles"]
    assert 0.0 < info["mean_fill"] <= info["max_fill"] <= 1.0
    nbr = TE.adjacency(ts)
    owner = np.full(sc.n_tets, -1)
    for t, T in enumerate(TE.plan_tiles(ts)):
        own = _owned(T, info["slots_per_thread"])
        assert own.size == T["n_owned"] > 0
        assert np.all(owner[own] == -1)
        owner[own] = t
        assert T["s_pad"] <= 2 * 768 and T["n_verts"] <= 1023 and T["rec_base"] + 48 * T["s_pad"] <= LDS[name]
        assert _face_connected(own, nbr)
    assert np.all(owner >= 0)
    assert info["lds_bytes"] <= LDS[name] and info["block_threads"] <= 768


@pytest.mark.parametrize("name", ["kuhn8", "kuhn10", "aveg"])
def test_refined_plan_replays_to_oracle(name, inputs, plans):
    sc, ts = inputs[name], plans[name]
    cache = O.prepare(sc.rest, sc.tets)
    x = scenes.deform(sc, 0.3)
    E, Es, Eb, g = O.energy_and_grad(x, cache, 5e-5, 2e-4, 4, grad_output=0.5)
    E2, Es2, Eb2, g2 = TE.emulate(ts, x, 5e-5, 2e-4, 4, grad_output=0.5)
    assert abs(E - E2) <= 1e-12 * abs(E)
    assert abs(Es - Es2) <= 1e-12 * Es and abs(Eb - Eb2) <= 1e-12 * max(Eb, 1e-300)
    assert np.abs(g - g2).max() <= 1e-11 * np.abs(g).max()


@pytest.mark.parametrize("name", ["kuhn8", "kuhn10", "aveg"])
def test_plan_bytes_do_not_depend_on_host_threads_or_the_run(name, inputs, plans):
    sc = inputs[name]
    ref = _plan_bytes(plans[name])
    assert _plan_bytes(_plan(sc, num_threads=1, **KW[name])) == ref
    assert _plan_bytes(_plan(sc, num_threads=8, **KW[name])) == ref


@pytest.mark.parametrize("name", ["kuhn8", "kuhn10", "aveg"])
def test_never_more_slots_and_staged_rows_than_the_parent(name, plans):
    info = plans[name].plan_info()
    print(name, "slots + staged rows:", info["total_slots"] + info["shared_vertex_copies"], "parent:", PARENT[name],
          "kept the bisection:", info["bisection_components"])
    assert info["total_slots"] + info["shared_vertex_copies"] <= PARENT[name]
    assert info["bisection_components"] in (0, 1)


def _grid_template():
    """A kuhn10 ball whose coordinates are multiples of 2^-10: copies scaled by a power of two and moved by multiples of 2^-6 are
    exact in fp32, so a copy's cut on its own has to equal the cut it takes over from the template."""
    v, t = scenes.kuhn_ball(10)
    return np.round(v * 1024.0) / 1024.0, t


def test_copies_of_a_template_take_its_cut():
    v, t = _grid_template()
    nv = v.shape[0]
    a = (v * 0.5 + np.array([-1.25, 0.5, 0.0])).astype(np.float32)
    b = (v * 2.0 + np.array([3.0, -2.0, 1.5])).astype(np.float32)
    assert np.array_equal(a.astype(np.float64), v * 0.5 + np.array([-1.25, 0.5, 0.0]))
    kw = dict(lds_budget_bytes=40000)
    both = _plan(scenes.TetScene(rest=np.concatenate([a, b]), tets=np.concatenate([t, t + nv]).astype(np.int32),
                                 sphere_vertex_offsets=np.array([0, nv, 2 * nv]), sphere_tet_offsets=np.array([0, len(t), 2 * len(t)]),
                                 radii=np.array([0.5, 2.0])), **kw)
    info = both.plan_info()
    assert info["cut_components"] == 2 and info["cut_templates"] == 1 and info["bisection_components"] == 0
    alone = []
    for k, rest in enumerate((a, b)):
        ts = _plan(scenes.TetScene(rest=rest, tets=t, sphere_vertex_offsets=np.array([0, nv]), sphere_tet_offsets=np.array([0, len(t)]),
                                   radii=np.array([1.0])), **kw)
        assert ts.plan_info()["cut_templates"] == 1
        alone += [c + k * len(t) for c in _cells(ts)]
    cells = _cells(both)
    assert len(cells) == len(alone) >= 8
    for c, d in zip(cells, alone):
        assert np.array_equal(c, d)


def test_a_permuted_tet_makes_another_template():
    v, t = _grid_template()
    nv = v.shape[0]
    a = v.astype(np.float32)
    b = (v + np.array([4.0, 0.0, 0.0])).astype(np.float32)
    t2 = t.copy()
    t2[100] = t2[100][[1, 2, 0, 3]]          # the same tet, the same orientation, another vertex order
    sc = scenes.TetScene(rest=np.concatenate([a, b]), tets=np.concatenate([t, t2 + nv]).astype(np.int32),
                         sphere_vertex_offsets=np.array([0, nv, 2 * nv]), sphere_tet_offsets=np.array([0, len(t), 2 * len(t)]),
                         radii=np.array([1.0, 1.0]))
    info = _plan(sc, lds_budget_bytes=40000).plan_info()
    assert info["cut_components"] == 2 and info["cut_templates"] == 2
    # ... and so does a copy that is not similar: one vertex moved by a hundredth of the extent
    b2 = b.copy()
    b2[nv // 2] += np.float32(0.02)
    sc = scenes.TetScene(rest=np.concatenate([a, b2]), tets=np.concatenate([t, t + nv]).astype(np.int32),
                         sphere_vertex_offsets=np.array([0, nv, 2 * nv]), sphere_tet_offsets=np.array([0, len(t), 2 * len(t)]),
                         radii=np.array([1.0, 1.0]))
    assert _plan(sc, lds_budget_bytes=40000).plan_info()["cut_templates"] == 2
