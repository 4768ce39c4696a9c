"""The gradient tile kernels add up a tile's energy pair at the END of the tile (tile_kernel.hip: kSumLate, sum_waves): the wave sums
are published to the reduction scratch behind the H stores, and the last wave reads them back after its own vertex sums -- three
passes, a scatter and the per-vertex sums later, with the force array written over the records next to the scratch in between.

The shapes are the smallest at which that can go wrong: a last wave with inactive lanes and no vertex block (the usual case), a
workgroup of ONE wave (walker and reducer at once), a last wave that owns a vertex block, tiles with more vertices than lanes (the
extra rounds of the per-vertex sums run before the reduction) and a fat lane layout.  Per case and penalty order: the launch-argument
route (eager), the HIP-graph replay and the device coefficient buffer; repeats are bitwise equal, the three routes and the forward-only
kernel (which reduces around the barrier after pass 2, as before) give the same energy to the last bit, and energy, terms and gradient
lie within the tolerances tests/test_gpu_parity.py asserts against the float64 oracle."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EPS = 2.0 ** -23
GUARD_E, GUARD_G, GUARD_V = 40.0, 8.0, 30.0          # tests/test_gpu_parity.py: the regression guard factors


def _more_vertices_than_lanes(info):
    return info["max_tile_vertices"] > info["block_threads"]


# (scene, spheres, options, what the plan must look like for the case to be the one it claims to be)
CASES = {
    "last_wave_idle_in_sums": ("kuhn8", 2, dict(),
                               lambda i: i["n_tiles"] > 2 and i["shared_vertex_copies"] > 0 and i["block_threads"] > 64 and i["block_threads"] % 64 == 0
                               and i["max_tile_vertices"] <= i["block_threads"] - 64),
    "one_wave": ("kuhn3", 6, dict(max_threads=64), lambda i: i["block_threads"] == 64 and not _more_vertices_than_lanes(i)),
    "last_wave_owns_a_vertex_block": ("kuhn6", 2, dict(max_threads=128, lds_budget_bytes=40960),
                                      lambda i: i["block_threads"] == 128 and i["max_tile_vertices"] > 64 and not _more_vertices_than_lanes(i)),
    "extra_rounds": ("kuhn1", 40, dict(max_threads=64, lds_budget_bytes=16384), lambda i: i["block_threads"] == 64 and _more_vertices_than_lanes(i)),
    "fat_layout": ("kuhn8", 2, dict(slots_per_thread=3), lambda i: i["slots_per_thread"] == 3 and i["shared_vertex_copies"] > 0 and i["block_threads"] > 64),
    "fat_layout_extra_rounds": ("kuhn8", 2, dict(slots_per_thread=3, max_threads=64),
                                lambda i: i["slots_per_thread"] == 3 and i["block_threads"] == 64 and _more_vertices_than_lanes(i) and i["shared_vertex_copies"] > 0),
}


@pytest.fixture(scope="module")
def oracle_cache():
    """float64 oracle values per (case, order): computed once, shared by the routes."""
    return {}


def _reference(oracle_cache, case, order):
    from oracle import tet_energy_oracle as O
    from tssplat_amd import scenes
    key = (case, order)
    if key not in oracle_cache:
        kind, S, _, _ = CASES[case]
        sc = scenes.make_scene(kind, S)
        x = scenes.deform(sc, 0.3)                       # many inverted tets: both energy terms live
        c1, c2, go = 2e-4 / S, 2e-4, 0.37
        cache = O.prepare(sc.rest, sc.tets)
        E, Es, Eb, g = O.energy_and_grad(x, cache, c1, c2, order, grad_output=go)
        assert Es > 0 and Eb > 0
        tol_e, tol_g = O.factored_tolerances(x, cache, c1, c2, order)
        A, nMx = O.tolerance_scales(x, cache)
        std_e, std_gv = O.rounding_error_model(x, cache, c1, c2, order)
        oracle_cache[key] = dict(sc=sc, x=x, c1=c1, c2=c2, go=go, E=E, Es=Es, Eb=Eb, g=g, tol_e=tol_e, tol_g=tol_g, A=A, nMx=nMx, std_e=std_e, std_gv=std_gv)
    return oracle_cache[key]


def _assert_parity(label, r, e_gpu, g_gpu, terms):
    """The assertions of tests/test_gpu_parity.py::_assert_parity on values already computed."""
    c1, c2, go, E, g = r["c1"], r["c2"], r["go"], r["E"], r["g"]
    g_gpu = g_gpu.astype(np.float64)
    band_e = 1e-5 * abs(E) + 8 * EPS * float(np.float32(c1)) * r["A"] + 1e-5 * float(np.float32(c2)) * r["Eb"]
    band_g = abs(go) * (1e-5 * np.linalg.norm(g / go) + 8 * EPS * float(np.float32(c1)) * r["nMx"])
    err_e, err_g = abs(e_gpu - E), float(np.linalg.norm(g_gpu - g))
    std_g = abs(go) * float(np.sqrt(np.sum(r["std_gv"] ** 2)))
    err_v = np.linalg.norm(g_gpu - g, axis=1)
    floor_v = abs(go) * (r["std_gv"] + 1e-3 * float(np.sqrt(np.mean(r["std_gv"] ** 2))))
    ratio_v = float(np.max(err_v / np.maximum(floor_v, 1e-300)))
    print(f"[{label}] E={E:.6e} gpu={e_gpu:.6e} err={err_e:.2e} tol={r['tol_e']:.2e} | |g|={np.linalg.norm(g):.4e} err={err_g:.2e} tol={abs(go) * r['tol_g']:.2e} | "
          f"guard ratios err/std: E {err_e / max(r['std_e'], 1e-300):.2f} g {err_g / max(std_g, 1e-300):.2f} vertex-max {ratio_v:.2f}")
    assert np.isfinite(e_gpu) and np.isfinite(g_gpu).all()
    assert err_e <= r["tol_e"] and err_g <= abs(go) * r["tol_g"], label
    assert err_e <= band_e + r["tol_e"] and err_g <= band_g + abs(go) * r["tol_g"], label
    assert err_e <= GUARD_E * r["std_e"] and err_g <= GUARD_G * std_g and ratio_v <= GUARD_V, label
    if terms is not None:
        assert abs(terms[0] - r["Es"]) <= r["tol_e"] / max(float(np.float32(c1)), 1e-30) + 1e-12 + 1e-6 * abs(r["Es"]), label
        assert abs(terms[1] - r["Eb"]) <= 2e-5 * r["Eb"] + 1e-12 + r["tol_e"] / max(float(np.float32(c2)), 1e-30), label


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("case", list(CASES))
def test_energy_pair_reduced_at_the_end_of_the_tile(oracle_cache, case, order):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from tssplat_amd import _capi, tet_spheres_ext as ext
    from tssplat_amd.energies import SmoothnessBarrierEnergy, GraphedSmoothnessBarrier
    lib = _capi.load()
    kind, S, kw, plan_ok = CASES[case]
    r = _reference(oracle_cache, case, order)
    sc, c1, c2, go = r["sc"], r["c1"], r["c2"], r["go"]

    class Flags:
        smooth_eng_coeff, barrier_coeff, increase_order_iter = c1, c2, 1000

    mod = SmoothnessBarrierEnergy(sc.rest, sc.tets, Flags, **kw)
    ts = mod.tet_sp
    info = ts.plan_info()
    assert plan_ok(info), info
    x = torch.from_numpy(r["x"]).cuda()
    go_dev = torch.tensor([go], dtype=torch.float32, device="cuda")
    stream = ext._stream_ptr(x.device)

    # coefficients as launch arguments, twice
    eager = []
    for _ in range(2):
        e = torch.full((), float("nan"), dtype=torch.float32, device="cuda")
        g = torch.full_like(x, float("nan"))
        _capi.check(lib.tsamd_forward_backward(ts._handle(), x.data_ptr(), go_dev.data_ptr(), c1, c2, order, stream, e.data_ptr(), g.data_ptr()))
        eager.append((_bits(e), ts.energy_terms(), _bits(g), float(e), g.cpu().numpy()))
    assert eager[0][:3] == eager[1][:3], "two evaluations differ"
    _assert_parity(f"{case} p={order} eager", r, eager[0][3], eager[0][4], eager[0][1])

    # HIP-graph replay, twice
    graphed = GraphedSmoothnessBarrier(mod, x, grad_scale=go)
    replay = []
    for _ in range(2):
        e_rep, g_rep = graphed.evaluate(c1, c2, order)
        replay.append((_bits(e_rep), ts.energy_terms(), _bits(g_rep), float(e_rep), g_rep.cpu().numpy()))
    assert replay[0][:3] == replay[1][:3], "two replays differ"
    assert replay[0][0] == eager[0][0] and replay[0][1] == eager[0][1], (replay[0][3], eager[0][3])
    _assert_parity(f"{case} p={order} replay", r, replay[0][3], replay[0][4], replay[0][1])

    # coefficients from the device buffer
    coef = torch.tensor([c1, c2], dtype=torch.float32, device="cuda")
    e_dev = torch.full((), float("nan"), dtype=torch.float32, device="cuda")
    g_dev = torch.full_like(x, float("nan"))
    _capi.check(lib.tsamd_evaluate_dev_coef(ts._handle(), x.data_ptr(), go_dev.data_ptr(), coef.data_ptr(), order, stream, e_dev.data_ptr(), g_dev.data_ptr()))
    terms_dev = ts.energy_terms()
    assert _bits(e_dev) == eager[0][0] and terms_dev == eager[0][1], (float(e_dev), eager[0][3])
    _assert_parity(f"{case} p={order} device coefficients", r, float(e_dev), g_dev.cpu().numpy(), terms_dev)

    # the forward-only kernel of the same layout (reduces around the barrier after pass 2): same wave sums, same butterfly
    e_fwd = ext.forward(x, ts, c1, c2, order, fuse=False)
    assert _bits(e_fwd) == eager[0][0] and ts.energy_terms() == eager[0][1], (float(e_fwd), eager[0][3])
