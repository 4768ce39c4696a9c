"""CPU tests of the partition of tet-spheres too large for one tile (tssplat_amd/csrc/partition.cpp).  Plans are built with
``host_only=True`` and ``max_threads=768``: an explicit tiling option keeps the fullest tiles that fit -- the path the
partitioner serves -- instead of the small-batch re-tiling.  No compute kernel runs here."""
import re

import numpy as np
import pytest

from oracle import tet_energy_oracle as O
from tssplat_amd import scenes
import tile_emulator as TE

FULL = dict(max_threads=768)


def _plan(sc, **kw):
    from tssplat_amd import tet_spheres_ext as ext
    return ext.TetSpheres(sc.rest.reshape(-1), sc.tets.reshape(-1), host_only=True, **{**FULL, **kw})


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


def test_every_tet_is_owned_once_every_tile_fits_and_is_face_connected():
    sc = scenes.make_scene("kuhn19", 2)
    ts = _plan(sc)
    info = ts.plan_info()
    nbr = TE.adjacency(ts)
    owner = np.full(sc.n_tets, -1)
    for t, T in enumerate(TE.plan_tiles(ts)):
        own = _owned(T, info["slots_per_thread"])
        assert own.size == T["n_owned"]
        assert np.all(owner[own] == -1)
        owner[own] = t
        assert T["s_pad"] <= 2 * 768 and T["n_verts"] <= 1023 and T["rec_base"] + 48 * T["s_pad"] <= 81920
        assert _face_connected(own, nbr)
    assert np.all(owner >= 0)


def _replays(sc, **kw):
    ts = _plan(sc, **kw)
    cache = O.prepare(sc.rest, sc.tets)
    x = scenes.deform(sc, 0.2, seed=7)
    E, Es, Eb, g = O.energy_and_grad(x, cache, 3e-5, 2e-4, 2, grad_output=0.5)
    E2, Es2, Eb2, g2 = TE.emulate(ts, x, 3e-5, 2e-4, 2, grad_output=0.5)
    assert abs(E - E2) <= 1e-12 * abs(E)
    assert abs(Es - Es2) <= 1e-12 * Es and abs(Eb - Eb2) <= 1e-12 * max(Eb, 1e-300)
    assert np.abs(g - g2).max() <= 1e-11 * np.abs(g).max()
    return ts


@pytest.mark.parametrize("kind,S", [("kuhn12", 1), ("kuhn19", 2), ("cone", 2), ("delaunay6000", 1)])
def test_partitioned_plan_replays_to_oracle(kind, S):
    _replays(scenes.make_scene(kind, S))


def test_partitioned_real_mesh_replays_to_oracle(aveg):
    rest, tets = aveg
    _replays(scenes.replicate_spheres(rest.astype(np.float64), tets, 2, seed=3))


def test_partition_does_not_depend_on_the_number_of_host_threads():
    sc = scenes.make_scene("delaunay2500", 3)
    a, b = (_plan(sc, num_threads=k) for k in (1, 8))
    n = 0
    for Ta, Tb in zip(TE.plan_tiles(a), TE.plan_tiles(b)):
        for k in ("planes", "gvid", "vdst", "slot_tet", "row_start"):
            assert np.array_equal(Ta[k], Tb[k]), k
        n += 1
    assert n == a.plan_info()["n_tiles"] == b.plan_info()["n_tiles"] > 3


def test_kuhn19_cells_carry_fewer_halo_slots_than_the_bisection(monkeypatch, capfd):
    """The bisection cuts a kuhn19 sphere into 38 tiles at 1.284 slots per tet; the cells need at most 37 at <= 1.262, with the
    same launch shape (768 threads, two workgroups' LDS per CU)."""
    monkeypatch.setenv("TSAMD_PLAN_TIMING", "1")
    info = _plan(scenes.make_scene("kuhn19", 4)).plan_info()
    assert re.search(r"partition: 4 cut components, 4 refined", capfd.readouterr().err)
    assert info["total_slots"] / info["n_tets"] <= 1.262
    assert info["n_tiles"] <= 4 * 37
    assert info["block_threads"] == 768 and info["lds_bytes"] <= 79680


def test_bisection_is_kept_where_the_cells_do_not_beat_it(monkeypatch, capfd):
    """kuhn8 spheres: three bisection tiles each, and three cells under the same LDS limit carry no fewer slots -- the plan keeps
    the bisection's tiles (the count tests/test_plan_host.py pins) and replays to the oracle."""
    monkeypatch.setenv("TSAMD_PLAN_TIMING", "1")
    ts = _replays(scenes.make_scene("kuhn8", 4))
    assert re.search(r"partition: 4 cut components, 0 refined, 4 keep the bisection", capfd.readouterr().err)
    assert ts.plan_info()["n_tiles"] == 12
