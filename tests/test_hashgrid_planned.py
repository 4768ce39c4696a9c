"""The planned route to the hash-grid encoding's dL/dparams (``GridEncoding.plan_points``: csrc/grid_kernels.hip, the
grid_plan_* / grid_planned_* kernels; contract in csrc/grid.h): a frozen point set is sorted once, every later backward is the
sorted route's segmented sum over the stored order.

CPU tier: the size queries, the C ABI's rejections and the methods' presence.  GPU tier: bitwise equality with the sorted route at
the sizes where its sort and sum change path, the float64 oracle's bound on its own, the forward's bits, plan ownership and reuse,
independence of plan / workspace placement through the C ABI, foreign plans, and the callers: ExplicitMaterial, a fit, and
MeshRasterizer with a view plan."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import hashgrid_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16,
           "per_level_scale": 1.447269237440378}
CONTENDED = {"otype": "HashGrid", "n_levels": 2, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16,
             "per_level_scale": 2.0}
SMALL = dict(DEFAULT, n_levels=4, log2_hashmap_size=12)


def _lay(cfg):
    return O.level_layout(cfg["n_levels"], cfg["n_features_per_level"], cfg["log2_hashmap_size"], cfg["base_resolution"],
                          cfg["per_level_scale"], cfg.get("otype") == "DenseGrid")


# ------------------------------------------------------------------------------------------------------------------ CPU tier
def test_plan_size_queries_without_a_gpu():
    from tssplat_amd import _capi
    lib = _capi.load()
    chunk = lib.tsamd_grid_sorted_chunk_points()
    s = C.c_float(1.447269237440378)

    def plan(n, F=2, L=16):
        out = C.c_int64(-1)
        assert lib.tsamd_grid_plan_bytes(n, L, F, 19, 16, s, 0, C.byref(out)) == 0
        return out.value

    def work(n, F=2, L=16):
        out = C.c_int64(-1)
        assert lib.tsamd_grid_backward_planned_workspace_bytes(n, L, F, 19, 16, s, 0, C.byref(out)) == 0
        return out.value
    ns = (0, 1, 63, 64, 65, 4099, 100_000, chunk - 1, chunk, chunk + 1, 3 * chunk + 5, 1 << 30)
    sizes = [plan(n) for n in ns]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[1] > 0        # monotone in n
    assert all(b >= n * 8 * 16 * 4 for n, b in zip(ns, sizes))
    assert plan(1000, L=4) >= 1000 * 8 * 4 * 4 and plan(1000, L=4) < plan(1000)
    assert plan(1000) == plan(1000)                                               # (n, config) only
    w = [work(n) for n in ns]
    assert all(a <= b for a, b in zip(w, w[1:])) and w[1] > 0
    assert w[-4] == w[-3] == w[-2] == w[-1]                                       # constant from one chunk on
    assert work(1000) == work(1000) and work(1000, F=8) >= work(1000)
    out = C.c_int64(0)
    for fn in (lib.tsamd_grid_plan_bytes, lib.tsamd_grid_backward_planned_workspace_bytes):
        assert fn(10, 16, 3, 19, 16, s, 0, C.byref(out)) == 1
        assert b"n_features_per_level" in lib.tsamd_last_error()
        assert fn(-1, 16, 2, 19, 16, s, 0, C.byref(out)) == 1
        assert b"n_points" in lib.tsamd_last_error()


def test_planned_c_abi_rejections_without_a_gpu():
    """Fake non-null pointers: every case fails before a launch."""
    from tssplat_amd import _capi
    lib = _capi.load()
    s = C.c_float(1.447269237440378)

    def q(fn, n, F=2, L=16):
        out = C.c_int64(-1)
        assert fn(n, L, F, 19, 16, s, 0, C.byref(out)) == 0
        return out.value
    plan_need = q(lib.tsamd_grid_plan_bytes, 10)
    sorted_need = q(lib.tsamd_grid_backward_sorted_workspace_bytes, 10)
    planned_need = q(lib.tsamd_grid_backward_planned_workspace_bytes, 10)

    def build(F=2, L=16, n=10, x=8, plan=256, plan_bytes=plan_need, ws=512, ws_bytes=sorted_need):
        return lib.tsamd_grid_plan_build(x, n, L, F, 19, 16, s, 0, plan, plan_bytes, ws, ws_bytes, None)

    def back(F=2, L=16, n=10, x=8, go=16, gp=16, plan=256, plan_bytes=plan_need, ws=512, ws_bytes=planned_need):
        return lib.tsamd_grid_encode_backward_planned(x, n, L, F, 19, 16, s, 0, go, gp, plan, plan_bytes, ws, ws_bytes, None)
    common = [(dict(plan=None), b"plan_dev is null"), (dict(plan=264), b"plan_dev is not aligned"),
              (dict(plan_bytes=plan_need - 1), b"plan_bytes"), (dict(ws=None), b"workspace_dev is null"),
              (dict(ws=520), b"workspace_dev is not aligned"), (dict(F=3), b"n_features_per_level"), (dict(L=0), b"n_levels"),
              (dict(n=-1), b"n_points"), (dict(x=None), b"x_dev")]
    for kw, msg in common + [(dict(ws_bytes=sorted_need - 1), b"workspace_bytes")]:
        assert build(**kw) == 1, kw
        assert msg in lib.tsamd_last_error(), (kw, lib.tsamd_last_error())
    for kw, msg in common + [(dict(ws_bytes=planned_need - 1), b"workspace_bytes"), (dict(go=None), b"grad_out_dev"),
                             (dict(gp=None), b"grad_params_dev"), (dict(gp=20), b"aligned")]:
        assert back(**kw) == 1, kw
        assert msg in lib.tsamd_last_error(), (kw, lib.tsamd_last_error())
    # nothing to do: no launch, no device, no buffers
    assert lib.tsamd_grid_plan_build(None, 0, 16, 2, 19, 16, s, 0, None, 0, None, 0, None) == 0
    assert lib.tsamd_grid_encode_backward_planned(None, 0, 16, 2, 19, 16, s, 0, None, None, None, 0, None, 0, None) == 0


def test_plan_points_has_no_cpu_fallback_and_the_callers_offer_plans():
    from tssplat_amd import encoding, materials, models, renderers, tcnn
    with pytest.raises(RuntimeError):
        encoding.GridEncoding(3, SMALL).plan_points(torch.zeros(4, 3))
    assert issubclass(tcnn.Encoding, encoding.GridEncoding) and callable(tcnn.Encoding.plan_points)
    for cls in (tcnn.NetworkWithInputEncoding, models.TCNNEncoding, models.ProgressiveBandHashGrid, models.CompositeEncoding,
                materials.ExplicitMaterial):
        assert callable(getattr(cls, "plan_points"))
    assert callable(renderers.MeshRasterizer.plan_views)
    assert encoding.plan_bytes(encoding.parse_grid_config(3, DEFAULT), 131_072) == 131_072 * 512


# ------------------------------------------------------------------------------------------------------------------ GPU tier
def _enc(cfg, P_np, param_grad="sorted"):
    from tssplat_amd import encoding
    enc = encoding.GridEncoding(3, cfg, param_grad=param_grad).cuda()
    with torch.no_grad():
        enc.params.copy_(torch.from_numpy(np.asarray(P_np, np.float32)))
    return enc


def _both(x_np, cfg, seed=0):
    """params.grad of the sorted route (by tensor) and of the planned route (by plan) for the same P, dy and x; and the inputs."""
    rng = np.random.default_rng(seed)
    lay = _lay(cfg)
    P = rng.uniform(-1, 1, lay["n_params"]).astype(np.float32)
    dy = rng.normal(size=(x_np.shape[0], lay["L"] * lay["F"])).astype(np.float32)
    x, dyd = torch.from_numpy(x_np).cuda(), torch.from_numpy(dy).cuda()
    a = _enc(cfg, P)
    a(x).backward(dyd)
    b = _enc(cfg, P)
    b(b.plan_points(x)).backward(dyd)
    assert float(a.params.grad.abs().max()) > 0
    return a.params.grad, b.params.grad, P, dy


def _assert_same_bits(x_np, cfg, seed=0):
    s, p, P, dy = _both(x_np, cfg, seed)
    assert torch.equal(p, s), (int((p != s).sum()), float((p - s).abs().max()))
    return p, P, dy


def _assert_oracle_bound(g, x, P, dy, cfg):
    lay = _lay(cfg)
    ref, _ = O.encode_backward(x, P, dy, lay)
    adds, _ = O.encode_backward(x, P, np.abs(dy), lay)
    err = np.abs(g.cpu().double().numpy() - ref)
    print(f"planned dL/dparams: N = {x.shape[0]}, max err {err.max():.3e}")
    assert np.all(err <= 2e-5 * adds + 1e-6), err.max()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 63, 64, 65, 4099])
def test_planned_equals_sorted_at_wave_and_tile_edges(N):
    x = np.random.default_rng(N).uniform(-0.02, 1.02, (N, 3)).astype(np.float32)
    g, P, dy = _assert_same_bits(x, SMALL, seed=N)
    if N == 4099:
        _assert_oracle_bound(g, x, P, dy, SMALL)                      # on its own, not through the sorted route


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one_pass", "three_passes", "dense_not_a_power_of_two"])
def test_planned_equals_sorted_at_every_key_width(name):
    if name == "one_pass":
        cfg, N = dict(DEFAULT, n_levels=4, log2_hashmap_size=4), 5_000
    elif name == "three_passes":
        cfg, N = dict(DEFAULT, n_levels=12, log2_hashmap_size=22), 20_000
    else:                                                             # `% entries` in the rebuilt key
        cfg, N = dict(DEFAULT, otype="DenseGrid", n_levels=4, base_resolution=5, per_level_scale=2.0), 20_000
        assert any(e & (e - 1) for e in _lay(cfg)["entries"].tolist())
    _assert_same_bits(np.random.default_rng(7).uniform(-0.02, 1.02, (N, 3)).astype(np.float32), cfg, seed=8)


@pytest.mark.gpu
@pytest.mark.parametrize("F", [1, 4, 8])
def test_planned_equals_sorted_at_every_feature_width(F):
    cfg = dict(DEFAULT, n_levels=6, n_features_per_level=F, log2_hashmap_size=14)
    _assert_same_bits(np.random.default_rng(F).uniform(-0.05, 1.05, (40_000, 3)).astype(np.float32), cfg, seed=F)


@pytest.mark.gpu
def test_planned_equals_sorted_on_long_runs_and_run_carries():
    """60 000 points in one level-0 cell: 8 runs of 60 000 records, each spanning about 117 wave ranges; random and lexsorted."""
    x = np.random.default_rng(11).uniform(0.37, 0.43, (60_000, 3)).astype(np.float32)
    _assert_same_bits(x, CONTENDED, seed=12)
    order = np.lexsort((x[:, 0], x[:, 1], x[:, 2]))
    _assert_same_bits(np.ascontiguousarray(x[order]), CONTENDED, seed=13)


@pytest.mark.gpu
def test_planned_equals_sorted_over_more_than_one_chunk():
    from tssplat_amd import _capi
    N = _capi.load().tsamd_grid_sorted_chunk_points() + 777
    _assert_same_bits(np.random.default_rng(14).uniform(0, 1, (N, 3)).astype(np.float32), CONTENDED, seed=15)


@pytest.mark.gpu
def test_planned_default_config_equals_sorted_and_meets_the_oracle_bound():
    x = np.random.default_rng(2).uniform(-0.02, 1.02, (100_000, 3)).astype(np.float32)
    g, P, dy = _assert_same_bits(x, DEFAULT)
    _assert_oracle_bound(g, x, P, dy, DEFAULT)


@pytest.fixture(scope="module")
def small_case():
    """4099 points, the small config: x, P, ten dy, all on the GPU."""
    rng = np.random.default_rng(31)
    x = torch.from_numpy(rng.uniform(-0.02, 1.02, (4099, 3)).astype(np.float32)).cuda()
    P = rng.uniform(-1, 1, _lay(SMALL)["n_params"]).astype(np.float32)
    dys = [torch.from_numpy(rng.normal(size=(4099, 8)).astype(np.float32)).cuda() for _ in range(10)]
    return x, P, dys


@pytest.mark.gpu
def test_planned_forward_has_the_tensor_forwards_bits(small_case):
    x, P, _ = small_case
    enc = _enc(SMALL, P)
    plan = enc.plan_points(x)
    assert plan.n_points == 4099 and plan.nbytes >= 4099 * 8 * 4 * 4 and not plan.x.requires_grad
    assert plan.x.data_ptr() != x.data_ptr() and plan.x.is_contiguous()
    assert torch.equal(enc(plan), enc(x))


@pytest.mark.gpu
def test_the_plan_owns_its_points(small_case):
    x, P, dys = small_case
    enc = _enc(SMALL, P)
    mine = x.clone()
    plan = enc.plan_points(mine)
    out = enc(plan)
    out.backward(dys[0])
    want_out, want_grad = out.detach().clone(), enc.params.grad.clone()
    mine.uniform_(0, 1)                                               # the caller's tensor moves on; the plan does not
    enc.params.grad = None
    out = enc(plan)
    out.backward(dys[0])
    assert torch.equal(out, want_out) and torch.equal(enc.params.grad, want_grad)


@pytest.mark.gpu
def test_one_plan_serves_many_backwards(small_case):
    x, P, dys = small_case
    a, b = _enc(SMALL, P), _enc(SMALL, P, param_grad="atomic")        # (the plan is used whatever param_grad says)
    plan = b.plan_points(x)
    for dy in dys:
        a.params.grad = b.params.grad = None
        a(x).backward(dy)
        b(plan).backward(dy)
        assert torch.equal(b.params.grad, a.params.grad)


@pytest.mark.gpu
def test_planned_result_ignores_plan_and_workspace_placement():
    """Through the C ABI: the plan built into an 0xFF-filled buffer 256 B into a larger one, the backward with an 0xFF-filled
    displaced workspace, and again on a side stream: the same bits, the guard bytes untouched."""
    from tssplat_amd import _capi, encoding
    lib = _capi.load()
    cfg = encoding.parse_grid_config(3, DEFAULT)
    rng = np.random.default_rng(21)
    N = 20_000
    x = torch.from_numpy(rng.uniform(-0.02, 1.02, (N, 3)).astype(np.float32)).cuda()
    dy = torch.from_numpy(rng.normal(size=(N, 32)).astype(np.float32)).cuda()
    enc = encoding.GridEncoding(3, DEFAULT, param_grad="sorted").cuda()
    enc(enc.plan_points(x)).backward(dy)
    want = enc.params.grad
    args = encoding._args(cfg)
    pb, sb, wb = encoding.plan_bytes(cfg, N), encoding.sorted_workspace_bytes(cfg, N), encoding.planned_workspace_bytes(cfg, N)
    plan = torch.full((pb + 512,), 0xFF, dtype=torch.uint8, device="cuda")
    build_ws = torch.full((sb + 512,), 0xFF, dtype=torch.uint8, device="cuda")
    assert plan.data_ptr() % 256 == 0 and build_ws.data_ptr() % 256 == 0
    torch.cuda.synchronize()
    _capi.check(lib.tsamd_grid_plan_build(x.data_ptr(), N, *args, plan.data_ptr() + 256, pb, build_ws.data_ptr() + 256, sb, None))
    torch.cuda.synchronize()
    for buf, n in ((plan, pb), (build_ws, sb)):
        assert bool((buf[:256] == 0xFF).all()) and bool((buf[256 + n:] == 0xFF).all())
    side = torch.cuda.Stream()
    for stream in (None, side):
        ws = torch.full((wb + 512,), 0xFF, dtype=torch.uint8, device="cuda")
        grad = torch.zeros_like(want)
        torch.cuda.synchronize()
        _capi.check(lib.tsamd_grid_encode_backward_planned(x.data_ptr(), N, *args, dy.data_ptr(), grad.data_ptr(), plan.data_ptr() + 256, pb,
                                                           ws.data_ptr() + 256, wb, None if stream is None else stream.cuda_stream))
        torch.cuda.synchronize()
        assert torch.equal(grad, want)
        assert bool((ws[:256] == 0xFF).all()) and bool((ws[256 + wb:] == 0xFF).all())
        assert bool((plan[:256] == 0xFF).all()) and bool((plan[256 + pb:] == 0xFF).all())


@pytest.mark.gpu
def test_foreign_plans_are_refused_and_a_plan_carries_no_gradient_to_x(small_case):
    from tssplat_amd import encoding
    x, P, dys = small_case
    enc = _enc(SMALL, P)
    for other in (dict(SMALL, n_levels=5), dict(SMALL, n_features_per_level=4), dict(SMALL, log2_hashmap_size=13),
                  dict(SMALL, base_resolution=8), dict(SMALL, per_level_scale=2.0), dict(SMALL, otype="DenseGrid")):
        with pytest.raises(ValueError):
            enc(encoding.GridEncoding(3, other).cuda().plan_points(x))
    xg = x.clone().requires_grad_(True)
    out = enc(enc.plan_points(xg))
    out.backward(dys[0])
    assert xg.grad is None and enc.params.grad is not None


def _material(include_xyz, param_grad=None):
    from tssplat_amd import materials
    grid = dict(materials.ExplicitMaterial.Config(n_output_dims=3, material_activation="sigmoid").pos_encoding_config,
                n_levels=4, log2_hashmap_size=12, include_xyz=include_xyz)
    if param_grad is not None:
        grid["param_grad"] = param_grad
    torch.manual_seed(3)
    return materials.ExplicitMaterial({"n_output_dims": 3, "material_activation": "sigmoid", "pos_encoding_config": grid})


@pytest.mark.gpu
@pytest.mark.parametrize("include_xyz", [False, True])
def test_material_takes_a_plan(include_xyz):
    g = torch.Generator().manual_seed(4)
    pts = (torch.rand(1000, 3, generator=g) * 2 - 1).cuda()
    up = torch.randn(1000, 3, generator=g).cuda()
    planned, ref = _material(include_xyz), _material(include_xyz, param_grad="sorted")
    plan = planned.plan_points(pts)
    color = planned(positions=plan)["color"]
    assert torch.equal(color, planned(positions=pts)["color"])
    color.backward(up)
    ref(positions=pts)["color"].backward(up)
    a, b = planned.encoding.encoding.encoding.params.grad, ref.encoding.encoding.encoding.params.grad
    assert float(a.abs().max()) > 0 and torch.equal(a, b)


@pytest.mark.gpu
def test_a_planned_fit_equals_the_sorted_fit_bit_for_bit():
    """The fit of test_hashgrid_sorted.py::test_a_sorted_fit_repeats_bit_for_bit, once by tensor (sorted) and once with one plan."""
    from tssplat_amd import tcnn
    grid = {"otype": "HashGrid", "n_levels": 8, "n_features_per_level": 2, "log2_hashmap_size": 15, "base_resolution": 16,
            "per_level_scale": 1.447269237440378}
    mlp = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 1}
    g = torch.Generator().manual_seed(5)
    x = torch.rand(20_000, 3, generator=g).cuda()
    target = torch.rand(20_000, 3, generator=g).cuda()

    def fit(planned):
        model = tcnn.NetworkWithInputEncoding(3, 3, grid, mlp, seed=9, param_grad="sorted").cuda()
        inp = model.plan_points(x) if planned else x
        grads = []
        for _ in range(10):
            model.params.grad = None
            torch.nn.functional.l1_loss(model(inp), target).backward()
            grads.append(model.params.grad.clone())
            with torch.no_grad():
                model.params -= 10.0 * model.params.grad
        return grads, model.params.detach().clone(), model.n_network_params
    grads_a, params_a, n_net = fit(False)
    grads_b, params_b, _ = fit(True)
    assert float(grads_a[-1][n_net:].abs().max()) > 0
    for it, (a, b) in enumerate(zip(grads_a, grads_b)):
        assert torch.equal(a, b), it
    assert torch.equal(params_a, params_b)


def _renderer(optimize_geo=False):
    from tssplat_amd import geometry, materials, renderers
    m = np.load(os.path.join(ROOT, "tests", "golden", "mario_mesh.npz"))
    v, f = m["vertices"].astype(np.float32), m["faces"].astype(np.int32)
    geo = geometry.TetMeshGeometry(v, np.zeros((0, 4), np.int32), use_smooth_barrier=False, optimize_geo=optimize_geo,
                                   surface_vid=np.arange(v.shape[0], dtype=np.int32), surface_fid=f)
    grid = dict(materials.ExplicitMaterial.Config(n_output_dims=3, material_activation="sigmoid").pos_encoding_config,
                n_levels=4, log2_hashmap_size=12)
    torch.manual_seed(0)
    mat = materials.ExplicitMaterial({"n_output_dims": 3, "material_activation": "sigmoid", "pos_encoding_config": grid})
    return renderers.MeshRasterizer(geo, mat)


@pytest.mark.gpu
def test_renderer_with_a_view_plan(monkeypatch):
    from tssplat_amd import dr, scenes
    from tssplat_amd.utils.optimizer import AdamUniform
    views, res = 4, 64
    ren = _renderer()
    mvp = torch.from_numpy(scenes.dataset_mvps(views).astype(np.float32)).cuda()
    bg = torch.ones(views, res, res, 3, device="cuda")
    with pytest.raises(RuntimeError, match="frozen"):
        _renderer(optimize_geo=True).plan_views(mvp, res)
    plan = ren.plan_views(mvp, res)
    assert plan.n_points == int(plan.selector.sum()) > 100
    with torch.no_grad():
        plain = ren(mvp, only_alpha=False, iter_num=0, resolution=res, background=bg)["shaded"]
        assert torch.equal(ren(mvp, only_alpha=False, iter_num=0, resolution=res, background=bg, view_plan=plan)["shaded"], plain)
    with pytest.raises(RuntimeError, match="only_alpha"):
        ren(mvp, only_alpha=True, iter_num=0, resolution=res, background=bg, view_plan=plan)
    with pytest.raises(RuntimeError, match="permute_surface_scheduler"):
        ren(mvp, only_alpha=False, iter_num=0, resolution=res, background=bg, view_plan=plan, permute_surface_scheduler=lambda it: 0.01)
    target = (plain * 0.5).detach()

    def refuse(*a, **k):
        raise AssertionError("the planned forward must not rasterise or interpolate")
    monkeypatch.setattr(dr, "rasterize", refuse)
    monkeypatch.setattr(dr, "interpolate", refuse)
    opt = AdamUniform(ren.parameters(), lr=0.01)
    loss_fn = torch.nn.L1Loss()
    losses = []
    for it in range(20):
        out = ren(mvp, only_alpha=False, iter_num=it, resolution=res, background=bg, view_plan=plan,
                  permute_surface_scheduler=lambda it: None)
        loss = loss_fn(out["shaded"][..., :3], target[..., :3]) * 20
        opt.zero_grad(set_to_none=True)
        loss.backward()
        if it == 0:
            for p in ren.materials.parameters():
                assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
        opt.step()
        losses.append(float(loss))
    assert losses[-1] < losses[0], losses
