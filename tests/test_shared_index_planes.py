"""Shared index planes: the copies of one template read the template's index planes (planes 0-3) and row table.

Host side (no GPU): every tile of every copy names a representative in the first sphere whose bytes equal its own, the plan
still replays to the oracle, a batch of distinct meshes shares nothing, debug bit 2 makes every tile its own representative.
GPU side: sharing on and off give bit-identical energies and gradients, both within the factored tolerances of the oracle."""
import numpy as np
import pytest

from oracle import tet_energy_oracle as O
from tssplat_amd import scenes
import tile_emulator as TE

NO_SHARING = 4          # tsamd_options.debug_flags bit 2


@pytest.fixture(scope="module")
def ext():
    from tssplat_amd import tet_spheres_ext
    return tet_spheres_ext


def _concat(parts):
    """Several scenes as one batch (vertex ids re-based)."""
    rest, tets, radii, voff, toff = [], [], [], [0], [0]
    for sc in parts:
        tets.append(sc.tets + np.int32(voff[-1]))
        rest.append(sc.rest)
        radii.append(sc.radii)
        voff.extend(voff[-1] + sc.sphere_vertex_offsets[1:])
        toff.extend(toff[-1] + sc.sphere_tet_offsets[1:])
    return scenes.TetScene(rest=np.concatenate(rest), tets=np.concatenate(tets).astype(np.int32),
                           sphere_vertex_offsets=np.asarray(voff, np.int64), sphere_tet_offsets=np.asarray(toff, np.int64),
                           radii=np.concatenate(radii))


def _plan(ext, sc, **kw):
    return ext.TetSpheres(sc.rest.reshape(-1), sc.tets.reshape(-1), host_only=True, **kw)


def _assert_replays(ts, sc, round_fp32=True):
    cache = O.prepare(sc.rest, sc.tets, round_fp32=round_fp32)
    x = scenes.deform(sc, 0.3)
    E, Es, Eb, g = O.energy_and_grad(x, cache, 5e-5, 2e-4, 4, grad_output=0.5)
    E2, Es2, Eb2, g2 = TE.emulate(ts, x, 5e-5, 2e-4, 4, grad_output=0.5)
    assert abs(E - E2) <= 1e-12 * abs(E)
    assert abs(Es - Es2) <= 1e-12 * Es and abs(Eb - Eb2) <= 1e-12 * max(Eb, 1e-300)
    assert np.abs(g - g2).max() <= 1e-11 * np.abs(g).max()


SHAPE = ("n_slots", "n_owned", "s_pad", "n_verts", "n_rows", "rec_base")


def _assert_reps_carry_the_same_bytes(ts):
    tiles = list(TE.plan_tiles(ts))
    rep = ts.index_reps()
    assert len(rep) == len(tiles)
    for t, T in enumerate(tiles):
        R = tiles[rep[t]]
        assert rep[t] <= t and rep[rep[t]] == rep[t]                       # the first tile with these bytes, itself unshared
        assert all(T[k] == R[k] for k in SHAPE), (t, rep[t])
        assert np.array_equal(T["planes"][:4], R["planes"][:4]) and np.array_equal(T["row_start"], R["row_start"]), (t, rep[t])
    return tiles, rep


@pytest.mark.parametrize("kind,S", [("kuhn10", 4), ("aveg", 3)])
def test_every_tile_of_a_copy_shares_the_first_spheres_index_planes(ext, kind, S):
    sc = scenes.make_scene(kind, S)
    ts = _plan(ext, sc, max_threads=768)
    tiles, rep = _assert_reps_carry_the_same_bytes(ts)
    assert len(tiles) % S == 0
    per = len(tiles) // S
    assert per > 1                                                         # the spheres are cut: halo, lanes, ranks, colouring all in play
    nt = sc.n_tets // S
    for t, T in enumerate(tiles):                                          # sphere-major tiles: tile t belongs to sphere t // per
        own = T["slot_tet"][T["slot_tet"] >= 0]
        assert np.all(own // nt == t // per)
    unshared = [t for t in range(per, len(tiles)) if rep[t] >= per]
    assert not unshared, f"{len(unshared)} of {len(tiles) - per} tiles of the copies have no representative in the first sphere: {unshared[:8]}"
    assert np.array_equal(rep[:per], np.arange(per)) or np.all(rep[:per] < per)
    # a copy's tile holds the template tile's tets, slot for slot
    for t in range(per, len(tiles)):
        a, b = tiles[t]["slot_tet"], tiles[rep[t]]["slot_tet"]
        assert np.array_equal(a >= 0, b >= 0) and np.array_equal((a - (t // per) * nt)[a >= 0], (b - (rep[t] // per) * nt)[b >= 0])
    _assert_replays(ts, sc)


def test_debug_bit_makes_every_tile_its_own_representative(ext):
    sc = scenes.make_scene("kuhn10", 3)
    on, off = _plan(ext, sc, max_threads=768), _plan(ext, sc, max_threads=768, debug_flags=NO_SHARING)
    assert np.array_equal(off.index_reps(), np.arange(off.plan_info()["n_tiles"]))
    assert (on.index_reps() != np.arange(on.plan_info()["n_tiles"])).sum() == 2 * on.plan_info()["n_tiles"] // 3
    for Ta, Tb in zip(TE.plan_tiles(on), TE.plan_tiles(off)):              # the bit changes who is read, not what is there
        for k in ("planes", "gvid", "vdst", "slot_tet", "row_start"):
            assert np.array_equal(Ta[k], Tb[k]), k


def test_distinct_meshes_share_nothing(ext):
    sc = _concat([scenes.make_scene("delaunay1500", 1, seed=0), scenes.make_scene("delaunay1500", 1, seed=1),
                  scenes.make_scene("kuhn9", 1), scenes.make_scene("kuhn10", 1), scenes.make_scene("cone", 1)])
    ts = _plan(ext, sc, max_threads=768)
    rep = ts.index_reps()
    assert len(rep) > 5 and np.array_equal(rep, np.arange(len(rep)))
    _assert_replays(ts, sc)


@pytest.mark.parametrize("kw", [dict(), dict(rebuild_dminv=True), dict(slots_per_thread=3, max_threads=512), dict(lds_budget_bytes=40960, max_threads=512)])
def test_mixed_batch_shares_per_template_and_replays(ext, kw):
    """Copies between other meshes, small spheres packed several to a tile, hub vertices split into copies: whatever is shared
    carries the same bytes, the placed copies of the cut templates are shared in full, and the plan replays to the oracle."""
    sc = _concat([scenes.make_scene("kuhn10", 2, seed=1), scenes.make_scene("delaunay700", 1), scenes.make_scene("kuhn3", 12, seed=2),
                  scenes.make_scene("cone", 3, seed=3), scenes.make_scene("kuhn10", 1, seed=4)])
    ts = _plan(ext, sc, **kw)
    tiles, rep = _assert_reps_carry_the_same_bytes(ts)
    # tiles of the third kuhn10 sphere (the last component) are read at the first one's
    first = int(sc.sphere_tet_offsets[1]), int(sc.sphere_tet_offsets[-2])
    n_last = 0
    for t, T in enumerate(tiles):
        own = T["slot_tet"][T["slot_tet"] >= 0]
        if own.min() >= first[1]:
            n_last += 1
            assert tiles[rep[t]]["slot_tet"].max() < first[0], t
    assert n_last > 1
    _assert_replays(ts, sc, round_fp32=not kw.get("rebuild_dminv", False))


def test_sharing_does_not_depend_on_the_number_of_host_threads(ext):
    sc = scenes.make_scene("delaunay1500", 4)
    a, b = (_plan(ext, sc, num_threads=k) for k in (1, 8))
    assert np.array_equal(a.index_reps(), b.index_reps()) and (a.index_reps() != np.arange(len(a.index_reps()))).any()
    for Ta, Tb in zip(TE.plan_tiles(a), TE.plan_tiles(b)):
        for k in ("planes", "gvid", "vdst", "slot_tet", "row_start"):
            assert np.array_equal(Ta[k], Tb[k]), k


# ---- GPU: sharing on against sharing off (debug bit 2), and both against the oracle ----
torch = pytest.importorskip("torch")


def _eval(ext, ts, x_np, c1, c2, order, go):
    x = torch.from_numpy(x_np).cuda().requires_grad_(True)
    e = ext.forward(x, ts, c1, c2, order)
    g = ext.backward(torch.tensor(go), x, ts, c1, c2, order)
    return e.detach().cpu().numpy().copy(), g.cpu().numpy()


def _assert_on_equals_off_and_oracle(ext, sc, kw, sigma, order, L=None, min_shared=1):
    c1, c2, go = 2e-4 / max(sc.n_spheres, 1), 2e-4, 0.5
    x = scenes.deform(sc, sigma)
    opkw = dict(operator=L) if L is not None else {}
    on = ext.TetSpheres(sc.rest.reshape(-1), sc.tets.reshape(-1), **kw, **opkw)
    off = ext.TetSpheres(sc.rest.reshape(-1), sc.tets.reshape(-1), debug_flags=NO_SHARING, **kw, **opkw)
    rep_on, rep_off = on.index_reps(), off.index_reps()
    assert (rep_on != np.arange(len(rep_on))).sum() >= min_shared and np.array_equal(rep_off, np.arange(len(rep_off)))
    e_on, g_on = _eval(ext, on, x, c1, c2, order, go)
    e_off, g_off = _eval(ext, off, x, c1, c2, order, go)
    assert e_on.tobytes() == e_off.tobytes(), (float(e_on), float(e_off))
    assert g_on.tobytes() == g_off.tobytes(), float(np.abs(g_on - g_off).max())
    cache = O.prepare(sc.rest, sc.tets, L=L, round_fp32=not kw.get("rebuild_dminv", False))
    E, _, _, g = O.energy_and_grad(x, cache, c1, c2, order, grad_output=go)
    tol_e, tol_g = O.factored_tolerances(x, cache, c1, c2, order)
    err_e, err_g = abs(float(e_on) - E), float(np.linalg.norm(g_on.astype(np.float64) - g))
    print(f"[shared index {kw} s={sigma} p={order}] E={E:.6e} err={err_e:.2e} tol={tol_e:.2e} | |g|={np.linalg.norm(g):.4e} err={err_g:.2e} tol={go * tol_g:.2e}")
    assert np.isfinite(e_on) and np.isfinite(g_on).all()
    assert err_e <= tol_e and err_g <= go * tol_g
    return on, off


@pytest.mark.gpu
def test_gpu_placed_copies(ext):
    """6 x kuhn10, sigma = 0.3."""
    sc = scenes.make_scene("kuhn10", 6)
    on, _ = _assert_on_equals_off_and_oracle(ext, sc, {}, 0.3, 4)
    n = on.plan_info()["n_tiles"]
    assert (on.index_reps() != np.arange(n)).sum() == 5 * n // 6


@pytest.mark.gpu
def test_gpu_mixed_batch(ext):
    """kuhn10 copies, one Delaunay ball, kuhn8 spheres, and small spheres packed several to a tile."""
    sc = _concat([scenes.make_scene("kuhn10", 2, seed=1), scenes.make_scene("delaunay1500", 1), scenes.make_scene("kuhn8", 5, seed=2),
                  scenes.make_scene("kuhn3", 12, seed=5), scenes.make_scene("kuhn10", 1, seed=4)])
    _assert_on_equals_off_and_oracle(ext, sc, {}, 0.3, 2, min_shared=4)


@pytest.mark.gpu
def test_gpu_few_shared_tiles_among_distinct_meshes(ext):
    """Fewer than half of the tiles share: the plan keeps the non-temporal tile kernel, which reads the representatives all the same."""
    sc = _concat([scenes.make_scene("kuhn10", 2, seed=1), scenes.make_scene("delaunay1500", 1, seed=0), scenes.make_scene("delaunay1500", 1, seed=1),
                  scenes.make_scene("kuhn9", 1), scenes.make_scene("kuhn11", 1)])
    on, _ = _assert_on_equals_off_and_oracle(ext, sc, {}, 0.3, 4)
    rep = on.index_reps()
    assert 0 < 2 * (rep != np.arange(len(rep))).sum() < len(rep)


@pytest.mark.gpu
def test_gpu_cone_hub_vertices_split_into_copies(ext):
    sc = scenes.make_scene("cone", 3)
    _assert_on_equals_off_and_oracle(ext, sc, {}, 0.2, 2)


@pytest.mark.gpu
def test_gpu_explicit_operator(ext):
    sc = scenes.make_scene("kuhn10", 3)
    L = O.element_laplacian_scaled(O.face_adjacency(sc.tets))                  # not symmetric: row and column weights
    on, _ = _assert_on_equals_off_and_oracle(ext, sc, {}, 0.3, 4, L=L)
    assert on.plan_info()["n_planes"] == 22


@pytest.mark.gpu
def test_gpu_rebuild_dminv(ext):
    sc = scenes.make_scene("kuhn10", 3)
    on, _ = _assert_on_equals_off_and_oracle(ext, sc, dict(rebuild_dminv=True), 0.3, 4)
    assert on.plan_info()["n_planes"] == 4


@pytest.mark.gpu
def test_gpu_fat_wave_layout(ext):
    """3 slots per lane: planes that are not interleaved in pairs in the device image."""
    sc = scenes.make_scene("kuhn10", 3)
    _assert_on_equals_off_and_oracle(ext, sc, dict(slots_per_thread=3, max_threads=512), 0.3, 2)


@pytest.mark.gpu
def test_gpu_graph_replay_equals_eager(ext):
    """A HIP-graph replay over a shared plan against the eager evaluation of the same plan and of the unshared one."""
    from tssplat_amd.energies import SmoothnessBarrierEnergy, GraphedSmoothnessBarrier

    class Flags:
        smooth_eng_coeff = 2e-4 / 4
        barrier_coeff = 2e-4
        increase_order_iter = 1000

    sc = scenes.make_scene("kuhn10", 4)
    mod = SmoothnessBarrierEnergy(sc.rest, sc.tets, Flags)
    off = SmoothnessBarrierEnergy(sc.rest, sc.tets, Flags, debug_flags=NO_SHARING)
    assert (mod.tet_sp.index_reps() != np.arange(mod.tet_sp.plan_info()["n_tiles"])).any()
    x = torch.nn.Parameter(torch.from_numpy(scenes.deform(sc, 0.3)).cuda())
    graphed = GraphedSmoothnessBarrier(mod, x)
    for it in (0, 600, 1001):
        e_g, g_g = graphed.step(it)
        e_g, g_g = e_g.clone(), g_g.clone()
        c1, c2 = mod.coeff_scheduler(it)
        eager = []
        for m in (mod, off):
            x.grad = None
            e = m(x, it, c1, c2)
            e.backward()
            assert float(e_g) == float(e.detach()), (it, float(e_g), float(e.detach()))
            # (replay and eager route apply c1 and grad_output in different places: equal to rounding, like test_graph_replay_equals_eager)
            assert torch.allclose(g_g, x.grad, rtol=3e-7, atol=0), it
            eager.append(x.grad.clone())
        assert torch.equal(eager[0], eager[1]), it
