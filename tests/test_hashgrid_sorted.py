"""The sorted, atomic-free route to the hash-grid encoding's dL/dparams (``param_grad="sorted"``: csrc/grid_kernels.hip, the
grid_sorted_* kernels; contract in csrc/grid.h) against the float64 oracle tests/hashgrid_oracle.py.

CPU tier: the config key / keyword, the workspace query and the C ABI's rejections.  GPU tier: parity with the oracle within the
atomic route's bound at the sizes where the sort and the segmented sum change path (wave and tile edges, one to three radix
passes, non-power-of-two tables, every feature width, runs that span many sum blocks, more than one chunk), bitwise
repeatability (two calls, a side stream, a dirty and displaced workspace through the C ABI), dL/dx equal to the atomic route's,
and a fit that repeats bit for bit."""
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
             "per_level_scale": 2.0}                                  # the two coarse levels of test_backward_contended_coarse_levels


def _lay(cfg):
    return O.level_layout(cfg["n_levels"], cfg["n_features_per_level"], cfg["log2_hashmap_size"], cfg["base_resolution"],
                          cfg["per_level_scale"], cfg.get("otype") == "DenseGrid")


# ------------------------------------------------------------------------------------------------------------------ CPU tier
def test_param_grad_config_key_and_keyword():
    from tssplat_amd import encoding, tcnn
    assert encoding.parse_grid_config(3, DEFAULT)["param_grad"] == "atomic"
    for mode in ("atomic", "sorted"):
        assert encoding.parse_grid_config(3, dict(DEFAULT, param_grad=mode))["param_grad"] == mode
        assert encoding.parse_grid_config(3, DEFAULT, param_grad=mode)["param_grad"] == mode
    with pytest.raises(ValueError, match="param_grad"):
        encoding.parse_grid_config(3, dict(DEFAULT, param_grad="fast"))
    with pytest.raises(ValueError, match="param_grad"):
        encoding.parse_grid_config(3, DEFAULT, param_grad="fast")
    # the keyword wins over the config key
    assert encoding.parse_grid_config(3, dict(DEFAULT, param_grad="sorted"), param_grad="atomic")["param_grad"] == "atomic"
    assert tcnn.Encoding(3, dict(DEFAULT, n_levels=2, param_grad="atomic"), param_grad="sorted").cfg["param_grad"] == "sorted"
    mlp = {"otype": "FullyFusedMLP", "n_neurons": 16, "n_hidden_layers": 1}
    small = dict(DEFAULT, n_levels=2)
    assert tcnn.NetworkWithInputEncoding(3, 3, small, mlp, param_grad="sorted").encoding_cfg["param_grad"] == "sorted"
    assert tcnn.NetworkWithInputEncoding(3, 3, dict(small, param_grad="sorted"), mlp).encoding_cfg["param_grad"] == "sorted"
    assert tcnn.NetworkWithInputEncoding(3, 3, small, mlp).encoding_cfg["param_grad"] == "atomic"


def test_sorted_encoding_module_builds_on_the_cpu():
    from tssplat_amd import encoding, tcnn
    a, b = encoding.GridEncoding(3, DEFAULT, param_grad="sorted"), tcnn.Encoding(3, DEFAULT)
    assert a.n_output_dims == 32 and a.params.shape == (12_599_920,) and a.params.dtype == torch.float32
    assert torch.equal(a.params.detach(), b.params.detach())          # the mode does not touch the initialisation
    assert "param_grad=sorted" in a.extra_repr() and "param_grad=atomic" in b.extra_repr()
    with pytest.raises(RuntimeError):
        a(torch.zeros(4, 3))                                          # no CPU fallback


def test_sorted_c_abi_without_a_gpu():
    from tssplat_amd import _capi
    lib = _capi.load()
    chunk = lib.tsamd_grid_sorted_chunk_points()
    assert chunk >= 1 << 16 and chunk & (chunk - 1) == 0
    s = C.c_float(1.447269237440378)

    def need(n, F=2, L=16):
        out = C.c_int64(-1)
        assert lib.tsamd_grid_backward_sorted_workspace_bytes(n, L, F, 19, 16, s, 0, C.byref(out)) == 0
        return out.value
    sizes = [need(n) for n in (0, 1, 63, 64, 65, 4099, 100_000, chunk - 1, chunk, chunk + 1, 3 * chunk + 5, 1 << 30)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[1] > 0
    assert sizes[-4] == sizes[-3] == sizes[-2] == sizes[-1]           # constant from one chunk on
    assert need(1000) == need(1000)                                   # n_points and the config only
    assert need(1000, F=8) >= need(1000)
    assert need(chunk) >= chunk * 8 * 8                               # room for every (point, corner) record
    out = C.c_int64(0)
    assert lib.tsamd_grid_backward_sorted_workspace_bytes(10, 16, 3, 19, 16, s, 0, C.byref(out)) == 1
    assert b"n_features_per_level" in lib.tsamd_last_error()
    assert lib.tsamd_grid_backward_sorted_workspace_bytes(-1, 16, 2, 19, 16, s, 0, C.byref(out)) == 1

    def back(F=2, L=16, gp=16, ws=256, ws_bytes=None, go=16, n=10):   # fake non-null pointers: every case fails before a launch
        nbytes = need(max(n, 0)) if ws_bytes is None else ws_bytes
        return lib.tsamd_grid_encode_backward_sorted(8, n, 16, L, F, 19, 16, s, 0, go, gp, None, ws, nbytes, None)
    for kw, msg in [(dict(ws=None), b"workspace_dev is null"), (dict(ws_bytes=need(10) - 1), b"workspace_bytes"),
                    (dict(ws=264), b"aligned"), (dict(F=3), b"n_features_per_level"), (dict(L=0), b"n_levels"),
                    (dict(go=None), b"grad_out_dev"), (dict(gp=20), b"aligned"), (dict(n=-1), b"n_points")]:
        assert back(**kw) == 1, kw
        assert msg in lib.tsamd_last_error(), (kw, lib.tsamd_last_error())
    # nothing to do: no launch, no device and no workspace needed
    assert lib.tsamd_grid_encode_backward_sorted(None, 0, 16, 16, 2, 19, 16, s, 0, None, 16, None, None, 0, None) == 0


# ------------------------------------------------------------------------------------------------------------------ GPU tier
def _grads(x_np, P_np, cfg, dy_np, param_grad="sorted", want_x=True):
    """(dL/dparams, dL/dx) of the HIP encoding as float32 GPU tensors."""
    from tssplat_amd import encoding
    enc = encoding.GridEncoding(3, cfg, param_grad=param_grad).cuda()
    with torch.no_grad():
        enc.params.copy_(torch.from_numpy(np.asarray(P_np, np.float32)))
    x = torch.from_numpy(np.asarray(x_np, np.float32)).cuda().requires_grad_(want_x)
    enc(x).backward(torch.from_numpy(np.asarray(dy_np, np.float32)).cuda())
    return enc.params.grad, (x.grad if want_x else None)


def _check_backward(x, cfg, seed=0, atol_rel=2e-5):
    """tests/test_hashgrid.py::_check_backward with param_grad="sorted": the same oracle and the same bound."""
    rng = np.random.default_rng(seed)
    lay = _lay(cfg)
    P = rng.uniform(-1, 1, lay["n_params"]).astype(np.float32)
    dy = rng.normal(size=(x.shape[0], lay["L"] * lay["F"])).astype(np.float32)
    gP, gx = _grads(x, P, cfg, dy)
    gP, gx = gP.cpu().double().numpy(), gx.cpu().double().numpy()
    rP, rx = O.encode_backward(x, P, dy, lay)
    absP, _ = O.encode_backward(x, P, np.abs(dy), lay)               # the sum of |adds| per entry: the fp32 summation scale
    err = np.abs(gP - rP)
    print(f"sorted dL/dparams: N = {x.shape[0]}, max err {err.max():.3e}, max err / (sum|adds| + 1e-30) "
          f"{(err / (absP + 1e-30))[absP > 0].max() if (absP > 0).any() else 0.0:.3e}")
    assert np.all(err <= atol_rel * absP + 1e-6), err.max()
    scale = np.abs(rx).max()
    bad = np.abs(gx - rx) > 1e-4 * scale + 1e-5 * np.abs(rx)
    assert bad.any(axis=1).mean() <= 1e-4, (bad.sum(), np.abs(gx - rx).max(), scale)
    return absP


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 63, 64, 65, 4099])
def test_sorted_backward_wave_and_tile_edges(N):
    """Wrap-around cells (points outside [0, 1]^3), a tail tile, a partly filled and an empty tail wave."""
    cfg = dict(DEFAULT, n_levels=4, log2_hashmap_size=12)
    _check_backward(np.random.default_rng(N).uniform(-0.02, 1.02, (N, 3)).astype(np.float32), cfg, seed=N)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one_pass", "three_passes", "dense_not_a_power_of_two"])
def test_sorted_backward_key_widths(name):
    if name == "one_pass":                                            # 16 entries per level: one radix pass, massive duplication
        cfg, N = dict(DEFAULT, n_levels=4, log2_hashmap_size=4), 5_000
    elif name == "three_passes":                                      # 22 key bits on the fine levels
        cfg, N = dict(DEFAULT, n_levels=12, log2_hashmap_size=22), 20_000
    else:                                                             # res 5, 10, 20, 40: entries 128, 1000, 8000, 64000 (`% entries`)
        cfg, N = dict(DEFAULT, otype="DenseGrid", n_levels=4, base_resolution=5, per_level_scale=2.0), 20_000
        assert any(e & (e - 1) for e in _lay(cfg)["entries"].tolist())
    _check_backward(np.random.default_rng(7).uniform(-0.02, 1.02, (N, 3)).astype(np.float32), cfg, seed=8)


@pytest.mark.gpu
@pytest.mark.parametrize("F", [1, 4, 8])
def test_sorted_backward_features_per_level(F):
    cfg = dict(DEFAULT, n_levels=6, n_features_per_level=F, log2_hashmap_size=14)
    _check_backward(np.random.default_rng(F).uniform(-0.05, 1.05, (40_000, 3)).astype(np.float32), cfg, seed=F)


@pytest.mark.gpu
def test_sorted_backward_long_runs_and_run_carries():
    """60 000 points inside one cell of level 0 (scale 15: cell 6 is x in [5.5 / 15, 6.5 / 15)): every point hits the same 8
    entries, so each of the 8 runs is 60 000 records long and spans about 117 sum blocks; in random and in lexsorted order."""
    x = np.random.default_rng(11).uniform(0.37, 0.43, (60_000, 3)).astype(np.float32)
    absP = _check_backward(x, CONTENDED, seed=12)
    assert np.count_nonzero(absP[:4096 * 2]) == 16                    # 8 entries x F = 2 on level 0
    order = np.lexsort((x[:, 0], x[:, 1], x[:, 2]))
    _check_backward(np.ascontiguousarray(x[order]), CONTENDED, seed=13)


@pytest.mark.gpu
def test_sorted_backward_more_than_one_chunk():
    from tssplat_amd import _capi
    N = _capi.load().tsamd_grid_sorted_chunk_points() + 777
    rng = np.random.default_rng(14)
    x = rng.uniform(0, 1, (N, 3)).astype(np.float32)
    _check_backward(x, CONTENDED, seed=15)
    lay = _lay(CONTENDED)
    P = rng.uniform(-1, 1, lay["n_params"]).astype(np.float32)
    dy = rng.normal(size=(N, 4)).astype(np.float32)
    a, _ = _grads(x, P, CONTENDED, dy, want_x=False)
    b, _ = _grads(x, P, CONTENDED, dy, want_x=False)
    assert torch.equal(a, b)


def _mario_points(views=8, res=128):
    """tests/test_hashgrid.py::_mario_points: foreground surface points of the mario golden mesh, in pixel order, in [0, 1]^3."""
    from tssplat_amd import dr, scenes
    m = np.load(os.path.join(ROOT, "tests", "golden", "mario_mesh.npz"))
    v = torch.from_numpy(m["vertices"].astype(np.float32)).cuda()
    tri = torch.from_numpy(m["faces"].astype(np.int32)).cuda()
    mvp = torch.from_numpy(scenes.dataset_mvps(views).astype(np.float32)).cuda()
    pos = torch.matmul(torch.cat([v, torch.ones_like(v[:, :1])], 1), mvp.transpose(1, 2)).contiguous()
    rast, _ = dr.rasterize(dr.RasterizeCudaContext(), pos, tri, resolution=[res, res], grad_db=False)
    p, _ = dr.interpolate(v[None], rast, tri)
    return ((p[rast[..., 3] > 0] + 1) * 0.5).cpu().numpy().astype(np.float32)


@pytest.mark.gpu
def test_sorted_backward_default_config_random_points():
    _check_backward(np.random.default_rng(2).uniform(-0.02, 1.02, (100_000, 3)).astype(np.float32), DEFAULT)


@pytest.mark.gpu
def test_sorted_backward_default_config_surface_points():
    pts = _mario_points()
    assert pts.shape[0] > 10000
    _check_backward(pts, DEFAULT, seed=3)


@pytest.fixture(scope="module")
def pixel_like():
    """Default config, 200 000 points in lexsorted (pixel-like) order, and the sorted route's gradients on them."""
    rng = np.random.default_rng(21)
    x = rng.uniform(-0.02, 1.02, (200_000, 3)).astype(np.float32)
    x = np.ascontiguousarray(x[np.lexsort((x[:, 0], x[:, 1], x[:, 2]))])
    P = rng.uniform(-1, 1, _lay(DEFAULT)["n_params"]).astype(np.float32)
    dy = rng.normal(size=(x.shape[0], 32)).astype(np.float32)
    gP, gx = _grads(x, P, DEFAULT, dy)
    torch.cuda.synchronize()
    assert float(gP.abs().max()) > 0
    return x, P, dy, gP.clone(), gx.clone()


@pytest.mark.gpu
def test_sorted_backward_is_bitwise_repeatable_across_calls(pixel_like):
    x, P, dy, gP, _ = pixel_like
    again, _ = _grads(x, P, DEFAULT, dy)
    assert torch.equal(again, gP)


@pytest.mark.gpu
def test_sorted_backward_is_bitwise_repeatable_on_a_side_stream(pixel_like):
    x, P, dy, gP, gx = pixel_like
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again, again_x = _grads(x, P, DEFAULT, dy)
    side.synchronize()
    assert torch.equal(again, gP) and torch.equal(again_x, gx)


@pytest.mark.gpu
def test_sorted_backward_ignores_the_workspace_contents_and_place(pixel_like):
    """Through the C ABI: a workspace filled with 0xFF bytes, 256 bytes into a larger buffer."""
    from tssplat_amd import _capi, encoding
    lib = _capi.load()
    x, P, dy, gP, gx = pixel_like
    cfg = encoding.parse_grid_config(3, DEFAULT)
    xd, Pd, dyd = (torch.from_numpy(a).cuda() for a in (x, P, dy))
    need = encoding.sorted_workspace_bytes(cfg, x.shape[0])
    buf = torch.full((need + 512,), 0xFF, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    grad_p, grad_x = torch.zeros_like(Pd), torch.empty_like(xd)
    torch.cuda.synchronize()
    _capi.check(lib.tsamd_grid_encode_backward_sorted(xd.data_ptr(), x.shape[0], Pd.data_ptr(), *encoding._args(cfg), dyd.data_ptr(),
                                                      grad_p.data_ptr(), grad_x.data_ptr(), buf.data_ptr() + 256, need, None))
    torch.cuda.synchronize()
    assert torch.equal(grad_p, gP) and torch.equal(grad_x, gx)
    assert bool((buf[:256] == 0xFF).all()) and bool((buf[256 + need:] == 0xFF).all())      # nothing written outside the workspace


@pytest.mark.gpu
def test_sorted_route_leaves_grad_x_as_the_atomic_route_computes_it(pixel_like):
    x, P, dy, _, gx = pixel_like
    _, atomic_x = _grads(x, P, DEFAULT, dy, param_grad="atomic")
    assert torch.equal(atomic_x, gx)


@pytest.mark.gpu
def test_a_sorted_fit_repeats_bit_for_bit():
    """Two fits from the same seed: encoding + fused MLP, L1 loss to a fixed target, plain gradient descent (no optimiser in the
    claim): params.grad after every iteration and the final params are bitwise equal."""
    from tssplat_amd import tcnn
    grid = {"otype": "HashGrid", "n_levels": 8, "n_features_per_level": 2, "log2_hashmap_size": 15, "base_resolution": 16,
            "per_level_scale": 1.447269237440378}
    mlp = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 1}
    g = torch.Generator().manual_seed(5)
    x = torch.rand(20_000, 3, generator=g).cuda()
    target = torch.rand(20_000, 3, generator=g).cuda()

    def fit():
        model = tcnn.NetworkWithInputEncoding(3, 3, grid, mlp, seed=9, param_grad="sorted").cuda()
        grads = []
        for _ in range(10):
            model.params.grad = None
            torch.nn.functional.l1_loss(model(x), target).backward()
            grads.append(model.params.grad.clone())
            with torch.no_grad():
                model.params -= 10.0 * model.params.grad
        return grads, model.params.detach().clone(), model.n_network_params
    grads_a, params_a, n_net = fit()
    grads_b, params_b, _ = fit()
    assert float(grads_a[-1][n_net:].abs().max()) > 0                 # the table does get a gradient
    for it, (a, b) in enumerate(zip(grads_a, grads_b)):
        assert torch.equal(a, b), it
    assert torch.equal(params_a, params_b)
    assert not torch.equal(params_a, tcnn.NetworkWithInputEncoding(3, 3, grid, mlp, seed=9).params.detach().cuda())



@pytest.mark.gpu
def test_material_config_key_switches_the_route():
    """ExplicitMaterial.pos_encoding_config -> get_encoding -> TCNNEncoding -> tcnn.Encoding: the key alone, no code change."""
    from tssplat_amd import materials
    grid = dict(materials.ExplicitMaterial.Config(n_output_dims=3, material_activation="sigmoid").pos_encoding_config,
                n_levels=4, log2_hashmap_size=12, param_grad="sorted")
    mat = materials.ExplicitMaterial({"n_output_dims": 3, "material_activation": "sigmoid", "pos_encoding_config": grid})
    enc = mat.encoding.encoding.encoding
    assert enc.cfg["param_grad"] == "sorted"
    pts = torch.rand(1000, 3, device="cuda") * 2 - 1
    grads = []
    for _ in range(2):
        enc.params.grad = None
        mat(pts)["color"].sum().backward()
        grads.append(enc.params.grad.clone())
    assert float(grads[0].abs().max()) > 0 and torch.equal(grads[0], grads[1])
