"""Regular batches: a plan that is copies of one template addresses the template's vertex ids, destinations and finish lists and
adds each copy's constants (csrc/regular_batch.h; tile_kernel.hip: tile_entry; step_kernels.hip: finish_kernel).

Host side (no GPU): copies report the tiles of one sphere as their period; the kernels' arithmetic -- multiply-shift quotient,
template entry plus constant -- reproduces every id, destination and finish entry of the plan; anything short of exact copies
reports period 0.  GPU side: the regular path gives the same bits as the same plan with debug bit 3 set (every tile and finish
vertex reads its own entries), through every launch route."""
import ctypes as C

import numpy as np
import pytest

from tssplat_amd import scenes
import tile_emulator as TE

NO_REGULAR = 8          # tsamd_options.debug_flags bit 3


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


# max_threads=768 keeps the tiling large batches get: with all-default options a plan of <= 1 024 tiles is re-tiled for latency, and
# there every copy of a lattice sphere keeps its own bisection, whose leaves come in another order from copy to copy (not regular)
def _plan(ext, sc, **kw):
    kw.setdefault("max_threads", 768)
    return ext.TetSpheres(sc.rest.reshape(-1), sc.tets.reshape(-1), host_only=True, **kw)


def _divide(rb, t):
    """Copy and template tile of tile t the way the kernels form them (64-bit product, shift, multiply, subtract)."""
    c = (int(t) * rb["div_mul"]) >> rb["div_shift"]
    return c, int(t) - c * rb["period"]


@pytest.mark.parametrize("kind,S", [("kuhn10", 4), ("aveg", 3), ("kuhn19", 5)])
def test_copies_report_the_tiles_of_one_sphere_and_the_arithmetic_reproduces_the_plan(ext, kind, S):
    sc = scenes.make_scene(kind, S)
    ts = _plan(ext, sc)
    tiles = list(TE.plan_tiles(ts))
    rb = ts.regular_batch()
    assert len(tiles) % S == 0 and len(tiles) // S > 1                     # several tiles per sphere
    assert rb["period"] == len(tiles) // S and rb["copies"] == S, rb
    assert rb["V"] == sc.rest.shape[0] // S
    info = ts.plan_info()
    assert rb["S"] * S == info["shared_vertex_copies"] and rb["K"] * S == info["finish_vertices"] and rb["K"] > 0
    assert 0 < rb["div_mul"] < 2 ** 32 and 0 <= rb["div_shift"] < 64
    # the multiply-shift pair is integer division for every tile index
    for t in range(len(tiles)):
        assert _divide(rb, t) == (t // rb["period"], t % rb["period"]), t
    # every tile, every lane: the template's entry plus the copy's constant is the plan's own entry
    for t, T in enumerate(tiles):
        c, r = _divide(rb, t)
        R = tiles[r]
        assert T["n_verts"] == R["n_verts"], t
        assert np.array_equal(R["gvid"] + c * rb["V"], T["gvid"]), t
        row = R["vdst"].astype(np.int64)
        excl = row >= 0
        dest = np.where(excl, row + c * rb["V"], ~row + c * rb["S"])       # (tile_kernel.hip: vertex_sums)
        assert np.array_equal(excl, T["vdst"] >= 0), t
        assert np.array_equal(dest, np.where(excl, T["vdst"], ~T["vdst"])), t
    # every finish entry: a thread's template entry kk, walked over the copies (step_kernels.hip: finish_kernel)
    vid, off, _ = TE.finish_lists(ts)
    K = rb["K"]
    assert len(vid) == S * K and len(off) == S * K + 1
    for c in range(S):
        assert np.array_equal(vid[:K] + c * rb["V"], vid[c * K:(c + 1) * K]), c
        assert np.array_equal(off[:K] + c * rb["S"], off[c * K:(c + 1) * K]), c            # e0
        assert np.array_equal(off[1:K + 1] + c * rb["S"], off[c * K + 1:(c + 1) * K + 1]), c   # e1, the closing sentinel included


def test_debug_bit_reports_period_zero_and_leaves_the_plan_alone(ext):
    sc = scenes.make_scene("kuhn10", 3)
    on, off = _plan(ext, sc), _plan(ext, sc, debug_flags=NO_REGULAR)
    assert on.regular_batch()["period"] > 0
    assert off.regular_batch() == dict(period=0, copies=0, V=0, S=0, K=0, div_mul=0, div_shift=0)
    assert on.plan_info() == off.plan_info() and np.array_equal(on.index_reps(), off.index_reps())
    for Ta, Tb in zip(TE.plan_tiles(on), TE.plan_tiles(off)):
        for k in ("planes", "gvid", "vdst", "slot_tet", "row_start"):
            assert np.array_equal(Ta[k], Tb[k]), k
    # period 0: quotient 0, remainder the tile -- the kernels' addresses are the plan's own
    assert all(_divide(off.regular_batch(), t) == (0, t) for t in range(off.plan_info()["n_tiles"]))


def _permuted_tet(sc, S):
    """The last copy's middle tet with its first three vertices rotated (orientation kept)."""
    tets = sc.tets.copy()
    e = (S - 1) * (tets.shape[0] // S) + tets.shape[0] // (2 * S)
    tets[e] = tets[e][[1, 2, 0, 3]]
    return scenes.TetScene(rest=sc.rest, tets=tets, sphere_vertex_offsets=sc.sphere_vertex_offsets, sphere_tet_offsets=sc.sphere_tet_offsets,
                           radii=sc.radii)


@pytest.mark.parametrize("case", ["two_templates", "copies_then_one_odd_sphere", "one_tet_permuted", "single_sphere"])
def test_anything_but_exact_copies_reports_period_zero(ext, case):
    sc = {"two_templates": lambda: _concat([scenes.make_scene("kuhn10", 2, seed=1), scenes.make_scene("kuhn9", 2, seed=2)]),
          "copies_then_one_odd_sphere": lambda: _concat([scenes.make_scene("kuhn10", 3, seed=1), scenes.make_scene("delaunay700", 1)]),
          "one_tet_permuted": lambda: _permuted_tet(scenes.make_scene("kuhn10", 3), 3),
          "single_sphere": lambda: scenes.make_scene("kuhn10", 1)}[case]()
    ts = _plan(ext, sc)
    assert ts.plan_info()["n_tiles"] > 1
    assert ts.regular_batch() == dict(period=0, copies=0, V=0, S=0, K=0, div_mul=0, div_shift=0)


def test_null_arguments_are_rejected(ext):
    from tssplat_amd import _capi
    lib = _capi.load()
    out = (C.c_int64 * 7)()
    assert lib.tsamd_get_regular_batch(None, out) == 1
    ts = _plan(ext, scenes.make_scene("kuhn8", 1))
    assert lib.tsamd_get_regular_batch(ts._handle(), None) == 1


# ---- GPU: the regular path against the same plan with debug bit 3 set ----
torch = pytest.importorskip("torch")


def _every_route(ext, ts, x_np, order):
    """Energy and gradient bytes of one plan through every launch route: stream launches (host and device coefficients, forward
    only), and the library's graph replayed with new coefficients into its own and into a redirected gradient buffer."""
    from tssplat_amd import _capi
    lib = _capi.load()
    c1, c2 = 5e-5, 2e-4
    x = torch.from_numpy(x_np).cuda()
    h, stream = ts._handle(), ext._stream_ptr(x.device)
    scale = torch.full((1,), 0.75, dtype=torch.float32, device=x.device)
    coef = torch.tensor([c1, c2], dtype=torch.float32, device=x.device)
    out = {}

    def keep(name, e, g=None):
        torch.cuda.synchronize()
        out[name] = (e.cpu().numpy().tobytes(), None if g is None else g.cpu().numpy().tobytes())
        assert torch.isfinite(e).all() and (g is None or (torch.isfinite(g).all() and float(g.abs().max()) > 0)), name

    e, g = torch.zeros((), device=x.device), torch.full_like(x, -7.0)
    _capi.check(lib.tsamd_forward_backward(h, x.data_ptr(), scale.data_ptr(), c1, c2, order, stream, e.data_ptr(), g.data_ptr()))
    keep("forward_backward", e, g)
    e, g = torch.zeros((), device=x.device), torch.full_like(x, -7.0)
    _capi.check(lib.tsamd_evaluate_dev_coef(h, x.data_ptr(), scale.data_ptr(), coef.data_ptr(), order, stream, e.data_ptr(), g.data_ptr()))
    keep("device_coefficients", e, g)
    e = torch.zeros((), device=x.device)
    _capi.check(lib.tsamd_forward(h, x.data_ptr(), c1, c2, order, stream, e.data_ptr()))
    keep("forward_only", e)
    e, g_own, g_other = torch.zeros((), device=x.device), torch.full_like(x, -7.0), torch.full_like(x, -7.0)
    graph = C.c_void_p()
    _capi.check(lib.tsamd_graph_create(h, x.data_ptr(), scale.data_ptr(), order, e.data_ptr(), g_own.data_ptr(), C.byref(graph)))
    try:
        _capi.check(lib.tsamd_graph_launch(graph, c1, c2, stream))
        keep("graph_replay", e, g_own)
        g_own.fill_(-7.0)
        _capi.check(lib.tsamd_graph_launch_to(graph, 2 * c1, c2, stream, None, g_other.data_ptr()))
        keep("graph_redirected_gradient", e, g_other)
        assert torch.equal(g_own, torch.full_like(x, -7.0))
    finally:
        torch.cuda.synchronize()
        lib.tsamd_graph_destroy(graph)
    return out


def _assert_regular_equals_own_entries(ext, sc, kw, order=4, sigma=0.3, regular=True, L=None):
    opkw = dict(operator=L) if L is not None else {}
    on = ext.TetSpheres(sc.rest.reshape(-1), sc.tets.reshape(-1), **kw, **opkw)
    off = ext.TetSpheres(sc.rest.reshape(-1), sc.tets.reshape(-1), debug_flags=NO_REGULAR, **kw, **opkw)
    rb = on.regular_batch()
    assert (rb["period"] > 1 and rb["K"] > 0) if regular else rb["period"] == 0, rb   # several tiles per sphere, shared vertices
    assert off.regular_batch()["period"] == 0 and on.plan_info()["n_tiles"] == off.plan_info()["n_tiles"]
    x = scenes.deform(sc, sigma)
    a, b = _every_route(ext, on, x, order), _every_route(ext, off, x, order)
    for name in a:
        assert a[name][0] == b[name][0], (name, "energy")
        assert a[name][1] == b[name][1], (name, "gradient")
    assert a["forward_backward"] == a["graph_replay"]       # (same coefficients, same grad_output: the same kernels, replayed)
    return on


@pytest.mark.gpu
@pytest.mark.parametrize("kind,kw", [("kuhn10", dict(max_threads=768)), ("aveg", dict())])
def test_gpu_regular_path_gives_the_bits_of_the_plans_own_entries(ext, kind, kw):
    _assert_regular_equals_own_entries(ext, scenes.make_scene(kind, 3), kw)


@pytest.mark.gpu
def test_gpu_mixed_templates(ext):
    sc = _concat([scenes.make_scene("kuhn10", 2, seed=1), scenes.make_scene("delaunay1500", 1), scenes.make_scene("kuhn8", 3, seed=2),
                  scenes.make_scene("kuhn10", 1, seed=4)])
    _assert_regular_equals_own_entries(ext, sc, dict(), order=2, regular=False)


@pytest.mark.gpu
def test_gpu_rebuild_dminv(ext):
    on = _assert_regular_equals_own_entries(ext, scenes.make_scene("kuhn10", 3), dict(max_threads=768, rebuild_dminv=True))
    assert on.plan_info()["n_planes"] == 4


@pytest.mark.gpu
def test_gpu_explicit_operator(ext):
    from oracle import tet_energy_oracle as O
    sc = scenes.make_scene("kuhn10", 3)
    L = O.element_laplacian_scaled(O.face_adjacency(sc.tets))                  # not symmetric: row and column weights
    on = _assert_regular_equals_own_entries(ext, sc, dict(max_threads=768), L=L)
    assert on.plan_info()["n_planes"] == 22


@pytest.mark.gpu
def test_gpu_regular_path_against_the_oracle(ext):
    """The regular path on its own: energy and gradient within the factored tolerances of the float64 oracle."""
    from oracle import tet_energy_oracle as O
    sc = scenes.make_scene("kuhn10", 3)
    ts = ext.TetSpheres(sc.rest.reshape(-1), sc.tets.reshape(-1), max_threads=768)
    assert ts.regular_batch()["period"] > 1
    c1, c2, order, go = 2e-4 / 3, 2e-4, 4, 0.5
    x_np = scenes.deform(sc, 0.3)
    x = torch.from_numpy(x_np).cuda().requires_grad_(True)
    e = ext.forward(x, ts, c1, c2, order)
    g = ext.backward(torch.tensor(go), x, ts, c1, c2, order).cpu().numpy()
    cache = O.prepare(sc.rest, sc.tets)
    E, _, _, gref = O.energy_and_grad(x_np, cache, c1, c2, order, grad_output=go)
    tol_e, tol_g = O.factored_tolerances(x_np, cache, c1, c2, order)
    assert abs(float(e) - E) <= tol_e and float(np.linalg.norm(g.astype(np.float64) - gref)) <= go * tol_g
