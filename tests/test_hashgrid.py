"""Hash-grid encoding of the texture stage (tssplat_amd.encoding / tcnn / models / materials, csrc/grid_kernels.hip) against the
float64 oracle tests/hashgrid_oracle.py.

CPU tier: the level layout (oracle and tsamd_grid_layout), hand-computed index / hash values, the oracle's gradients against
finite differences, the C ABI's rejections, the config rejections, and the reference's own models / materials modules building
their encoding on tssplat_amd.tcnn.  GPU tier: forward, dL/dparams and dL/dx against the oracle, determinism, the adjoint
identity, a 120 x 512^2-sized call, and the texture stage end to end through MeshRasterizer."""
import ctypes as C
import importlib
import os
import sys
import types

import numpy as np
import pytest
import torch

import hashgrid_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
DEFAULT = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16,
           "per_level_scale": 1.447269237440378}                      # materials/explicit_material.py Config defaults
DEFAULT_ENTRIES = [4096, 13824, 39304, 117656, 357912] + [524288] * 11


def _lay(cfg):
    return O.level_layout(cfg["n_levels"], cfg["n_features_per_level"], cfg["log2_hashmap_size"], cfg["base_resolution"],
                          cfg["per_level_scale"], cfg.get("otype") == "DenseGrid")


def _c_layout(cfg):
    from tssplat_amd import encoding
    return encoding.grid_layout(encoding.parse_grid_config(3, cfg))


# ------------------------------------------------------------------------------------------------------------------ CPU tier
def test_default_layout_known_answer():
    lay = _lay(DEFAULT)
    assert lay["entries"].tolist() == DEFAULT_ENTRIES
    assert lay["is_hash"].tolist() == [False] * 5 + [True] * 11
    assert lay["n_params"] == 12_599_920 and lay["offset"][-1] == 6_299_960
    c = _c_layout(DEFAULT)
    assert c["n_params"] == 12_599_920
    assert np.array_equal(c["offset"], lay["offset"]) and np.array_equal(c["res"], lay["res"])
    assert np.array_equal(c["is_hash"], lay["is_hash"])
    assert np.allclose(c["scale"], lay["scale"], rtol=1e-6, atol=0)
    assert c["res"][0] == 16 and c["res"][-1] == 4096                 # level 15: float32 scale 4094.9985 -> res 4096


def test_layout_mixed_dense_and_hashed_levels():
    """res 8, 16, 32, 64 against T = 4096: level 1 has res^3 == T exactly (stride <= T: still the dense index)."""
    cfg = {"otype": "HashGrid", "n_levels": 4, "n_features_per_level": 4, "log2_hashmap_size": 12, "base_resolution": 8,
           "per_level_scale": 2.0}
    lay, c = _lay(cfg), _c_layout(cfg)
    assert lay["res"].tolist() == [8, 16, 32, 64] and c["res"].tolist() == [8, 16, 32, 64]
    assert lay["entries"].tolist() == [512, 4096, 4096, 4096]
    assert lay["is_hash"].tolist() == [False, False, True, True] and c["is_hash"].tolist() == [False, False, True, True]
    assert lay["n_params"] == c["n_params"] == (512 + 3 * 4096) * 4
    dense = _c_layout(dict(cfg, otype="DenseGrid"))                    # no cap, never hashed
    assert dense["n_params"] == (512 + 4096 + 32768 + 262144) * 4 and not dense["is_hash"].any()


def test_layout_float32_boundary():
    """scale and resolution are float32: per_level_scale 1.2609000205993652 (a float32 value) at base 16 gives level 15 a float32
    scale of 516.99994 (res 518); the same formula in float64 lands a hair above 517 (res 519)."""
    import math
    cfg = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16,
           "per_level_scale": 1.2609000205993652}
    f64 = 2 ** (15 * math.log2(1.2609000205993652)) * 16 - 1
    assert 517.0 < f64 < 517.000001 and math.ceil(f64) + 1 == 519
    lay, c = _lay(cfg), _c_layout(cfg)
    assert lay["scale"][15] < 517.0 and lay["res"][15] == 518 and c["res"][15] == 518
    assert np.array_equal(lay["res"], c["res"]) and lay["n_params"] == c["n_params"]


def test_index_and_hash_known_answers():
    M = 0xFFFFFFFF
    h = (7 * 1) ^ ((11 * 2654435761) & M) ^ ((13 * 805459861) & M)
    got = O.grid_index(np.array([[7, 11, 13]], np.uint64), 4096, 1 << 19, True)
    assert got[0] == h % (1 << 19)
    assert O.grid_index(np.array([[3, 5, 7]], np.uint64), 16, 4096, False)[0] == 3 + 5 * 16 + 7 * 256
    # a point slightly below 0 at level 0 (scale 15): pos = fmaf(15, -0.05, 0.5) = -0.25 -> cell 0xFFFFFFFF, frac 0.75
    cell, frac = O.cell_position(np.array([[-0.05, 0.5, 1.02]], np.float32), np.float32(15.0))
    assert cell[0].tolist() == [M, 8, 15] and abs(frac[0, 0] - 0.75) < 1e-6
    # the wrapped corner: dense index (2^32 - 1) + 8 * 16 + 15 * 256 in uint32, % 4096
    assert O.grid_index(np.array([[M, 8, 15]], np.uint64), 16, 4096, False)[0] == ((M + 8 * 16 + 15 * 256) & M) % 4096
    # hashed, wrapped: the uint32 products
    assert O.grid_index(np.array([[M, M, 2]], np.uint64), 4096, 1 << 19, True)[0] == \
        (M ^ ((M * 2654435761) & M) ^ ((2 * 805459861) & M)) % (1 << 19)


def test_oracle_gradients_against_finite_differences():
    rng = np.random.default_rng(0)
    cfg = {"otype": "HashGrid", "n_levels": 3, "n_features_per_level": 2, "log2_hashmap_size": 8, "base_resolution": 4,
           "per_level_scale": 2.0}
    lay = _lay(cfg)
    x = rng.uniform(-0.05, 1.05, (6, 3))
    P = rng.uniform(-1, 1, lay["n_params"])
    dy = rng.normal(size=(6, lay["L"] * lay["F"]))
    gP, gx = O.encode_backward(x, P, dy, lay, exact=True)
    L = lambda xx, pp: float(np.sum(O.encode(xx, pp, lay, exact=True) * dy))
    h = 1e-6
    for k in rng.choice(lay["n_params"], 40, replace=False):
        e = np.zeros_like(P)
        e[k] = h
        assert abs((L(x, P + e) - L(x, P - e)) / (2 * h) - gP[k]) < 1e-7
    for i in range(6):
        for d in range(3):
            e = np.zeros_like(x)
            e[i, d] = 1e-7
            fd = (L(x + e, P) - L(x - e, P)) / 2e-7
            assert abs(fd - gx[i, d]) < 1e-5 * max(1.0, abs(gx[i, d])), (i, d, fd, gx[i, d])


def test_c_abi_rejections_without_a_gpu():
    from tssplat_amd import _capi
    lib = _capi.load()
    ok = dict(L=16, F=2, T=19, base=16, s=C.c_float(1.447269237440378), dense=0)

    def enc(x=8, n=10, p=16, L=16, F=2, T=19, base=16, s=1.447269237440378, dense=0, out=16):
        return lib.tsamd_grid_encode(x, n, p, L, F, T, base, C.c_float(s), dense, out, None)

    for kw, msg in [(dict(F=3), b"n_features_per_level"), (dict(L=0), b"n_levels"), (dict(L=33), b"n_levels"),
                    (dict(T=31), b"log2_hashmap_size"), (dict(base=0), b"base_resolution"), (dict(s=0.5), b"per_level_scale"),
                    (dict(dense=2), b"dense"), (dict(n=-1), b"n_points"), (dict(p=None), b"params_dev"), (dict(x=None), b"x_dev"),
                    (dict(out=None), b"out_dev"), (dict(p=20), b"aligned"), (dict(out=4), b"aligned")]:
        assert enc(**kw) == 1, kw
        assert msg in lib.tsamd_last_error(), (kw, lib.tsamd_last_error())
    assert lib.tsamd_grid_encode_backward(8, 10, 16, 16, 2, 19, 16, C.c_float(1.5), 0, None, 16, None, None) == 1
    assert b"grad_out_dev" in lib.tsamd_last_error()
    assert lib.tsamd_grid_encode_backward(8, 10, 16, 16, 4, 19, 16, C.c_float(1.5), 0, 16, 8, None, None) == 1
    assert b"aligned" in lib.tsamd_last_error()
    assert lib.tsamd_grid_layout(16, 2, 19, 16, C.c_float(1.0e6), 0, None, None, None, None, None) == 1   # resolution overflow
    n = C.c_int64(0)
    assert lib.tsamd_grid_layout(16, 2, 19, 16, ok["s"], 0, None, None, None, None, C.byref(n)) == 0 and n.value == 12_599_920
    assert enc(n=0, x=None, out=None) == 0                            # nothing to do: no launch, no device needed


def test_config_rejections():
    from tssplat_amd import encoding, tcnn
    for cfg, n_in in [(dict(DEFAULT, otype="Grid", type="Tiled"), 3), (dict(DEFAULT, interpolation="Nearest"), 3),
                      (dict(DEFAULT, interpolation="Smoothstep"), 3), (DEFAULT, 2), (dict(DEFAULT, n_features_per_level=3), 3),
                      (dict(DEFAULT, otype="Frequency"), 3)]:
        with pytest.raises(ValueError):
            encoding.parse_grid_config(n_in, cfg)
    with pytest.raises(ValueError):
        tcnn.Encoding(3, DEFAULT, dtype=torch.float16)
    for cls in (tcnn.Network, tcnn.NetworkWithInputEncoding):
        with pytest.raises(NotImplementedError, match="VanillaMLP"):
            cls(3, 3, {})
    for cfg in (dict(DEFAULT, otype="Grid", type="Hash"), dict(DEFAULT, otype="Grid", type="Dense", n_levels=2), dict(DEFAULT, otype="DenseGrid", n_levels=2)):
        encoding.parse_grid_config(3, cfg)


def test_encoding_module_builds_on_the_cpu():
    """Construction needs no device (the layout is host code): parameters uniform in [-1e-4, 1e-4], seeded."""
    from tssplat_amd import tcnn
    a, b = tcnn.Encoding(3, DEFAULT, seed=7), tcnn.Encoding(3, DEFAULT, seed=7)
    assert a.n_output_dims == 32 and a.params.shape == (12_599_920,) and a.params.dtype == torch.float32
    assert torch.equal(a.params.detach(), b.params.detach()) and float(a.params.detach().abs().max()) <= 1e-4
    with pytest.raises(RuntimeError):
        a(torch.zeros(4, 3))                                          # no CPU fallback


@pytest.mark.skipif(not os.path.exists(os.path.join(REF, "materials", "explicit_material.py")),
                    reason="the reference checkout only exists in the authoring container")
def test_reference_material_builds_on_the_stand_in(monkeypatch):
    """The reference's unmodified models/networks.py and materials/explicit_material.py, with `tinycudann` bound to
    tssplat_amd.tcnn and omegaconf stubbed (as test_reference_modules.py does), torch.cuda.device patched out."""
    from tssplat_amd import tcnn
    omega = types.ModuleType("omegaconf")
    omega.DictConfig = dict

    class _Node(dict):
        __getattr__ = dict.get

    class OmegaConf:
        @staticmethod
        def structured(obj):
            import dataclasses
            return _Node({k: (_Node(v) if isinstance(v, dict) else v) for k, v in dataclasses.asdict(obj).items()})

        @staticmethod
        def to_container(cfg, resolve=True):
            return dict(cfg)
    omega.OmegaConf, omega.open_dict = OmegaConf, (lambda cfg: cfg)
    nvd = types.ModuleType("nvdiffrast")
    nvd.torch = types.ModuleType("nvdiffrast.torch")
    for name, mod in {"omegaconf": omega, "tinycudann": tcnn, "nvdiffrast": nvd, "nvdiffrast.torch": nvd.torch}.items():
        monkeypatch.setitem(sys.modules, name, mod)
    for name in [n for n in sys.modules if n.split(".")[0] in ("models", "materials", "utils")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.syspath_prepend(REF)

    class _NoDevice:
        def __init__(self, *a):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False
    monkeypatch.setattr(torch.cuda, "device", _NoDevice)
    try:
        cfg = importlib.import_module("utils.config")
        monkeypatch.setattr(cfg, "get_device", lambda: torch.device("cpu"))
        mat_mod = importlib.import_module("materials.explicit_material")
        monkeypatch.setattr(mat_mod, "get_device", lambda: torch.device("cpu"))
        assert mat_mod.__file__.startswith(REF)
        m = mat_mod.ExplicitMaterial({"n_output_dims": 3, "material_activation": "sigmoid"})
        enc = m.encoding.encoding.encoding
        assert isinstance(enc, tcnn.Encoding)
        assert m.encoding.n_output_dims == 32 and enc.params.numel() == 12_599_920
        shapes = [tuple(p.shape) for p in m.feature_network.parameters()]
        assert shapes == [(64, 32), (3, 64)]                            # VanillaMLP: 32 -> 64 -> 3, bias-free
    finally:
        for name in [n for n in sys.modules if n.split(".")[0] in ("models", "materials", "utils")]:
            del sys.modules[name]


# ------------------------------------------------------------------------------------------------------------------ GPU tier
def _run(x_np, P_np, cfg, dy_np=None, want_x=True):
    """(forward, dL/dparams, dL/dx) of the HIP encoding as numpy float64."""
    from tssplat_amd import encoding
    enc = encoding.GridEncoding(3, cfg).cuda()
    with torch.no_grad():
        enc.params.copy_(torch.from_numpy(np.asarray(P_np, np.float32)))
    x = torch.from_numpy(np.asarray(x_np, np.float32)).cuda().requires_grad_(want_x)
    y = enc(x)
    if dy_np is None:
        return y.detach().cpu().double().numpy(), None, None
    y.backward(torch.from_numpy(np.asarray(dy_np, np.float32)).cuda())
    gx = x.grad.cpu().double().numpy() if want_x else None
    return y.detach().cpu().double().numpy(), enc.params.grad.cpu().double().numpy(), gx


def _mario_points(views=8, res=128):
    """Foreground surface points, in pixel order, of the mario golden mesh under dataset cameras, mapped into [0, 1]^3 as
    contract_to_unisphere does (bbox [-1, 1]^3)."""
    from tssplat_amd import dr, scenes
    m = np.load(os.path.join(ROOT, "tests", "golden", "mario_mesh.npz"))
    v = torch.from_numpy(m["vertices"].astype(np.float32)).cuda()
    tri = torch.from_numpy(m["faces"].astype(np.int32)).cuda()
    mvp = torch.from_numpy(scenes.dataset_mvps(views).astype(np.float32)).cuda()
    pos = torch.matmul(torch.cat([v, torch.ones_like(v[:, :1])], 1), mvp.transpose(1, 2)).contiguous()
    rast, _ = dr.rasterize(dr.RasterizeCudaContext(), pos, tri, resolution=[res, res], grad_db=False)
    p, _ = dr.interpolate(v[None], rast, tri)
    return ((p[rast[..., 3] > 0] + 1) * 0.5).cpu().numpy().astype(np.float32)


def _check_forward(x, cfg, seed=0):
    lay = _lay(cfg)
    P = np.random.default_rng(seed).uniform(-1, 1, lay["n_params"]).astype(np.float32)
    y, _, _ = _run(x, P, cfg)
    ref = O.encode(x, P, lay)
    err = np.abs(y - ref).max()
    assert err <= 4e-6, err                                          # |y| <= 1: a few fp32 ulps of the 8-term sum


@pytest.mark.gpu
def test_forward_default_config_random_and_surface_points():
    rng = np.random.default_rng(1)
    _check_forward(rng.uniform(-0.02, 1.02, (200_000, 3)).astype(np.float32), DEFAULT)
    pts = _mario_points()
    assert pts.shape[0] > 10000
    _check_forward(pts, DEFAULT)


@pytest.mark.gpu
@pytest.mark.parametrize("F", [1, 2, 4, 8])
def test_forward_features_per_level(F):
    cfg = dict(DEFAULT, n_levels=8, n_features_per_level=F, log2_hashmap_size=15)
    _check_forward(np.random.default_rng(F).uniform(-0.05, 1.05, (50_000, 3)).astype(np.float32), cfg, seed=F)


@pytest.mark.gpu
def test_forward_is_bitwise_repeatable():
    from tssplat_amd import encoding
    enc = encoding.GridEncoding(3, DEFAULT).cuda()
    with torch.no_grad():
        enc.params.uniform_(-1, 1)
    x = torch.rand(300_000, 3, device="cuda")
    assert torch.equal(enc(x), enc(x))


def _check_backward(x, cfg, seed=0, atol_rel=2e-5):
    rng = np.random.default_rng(seed)
    lay = _lay(cfg)
    P = rng.uniform(-1, 1, lay["n_params"]).astype(np.float32)
    dy = rng.normal(size=(x.shape[0], lay["L"] * lay["F"])).astype(np.float32)
    _, gP, gx = _run(x, P, cfg, dy)
    rP, rx = O.encode_backward(x, P, dy, lay)
    absP, _ = O.encode_backward(x, P, np.abs(dy), lay)               # the sum of |adds| per entry: the fp32 summation scale
    assert np.all(np.abs(gP - rP) <= atol_rel * absP + 1e-6), np.abs(gP - rP).max()
    # dL/dx: a point whose cell differs between fmaf rounding paths would jump; none do at these sizes, but allow 1e-4 of them
    scale = np.abs(rx).max()
    bad = np.abs(gx - rx) > 1e-4 * scale + 1e-5 * np.abs(rx)
    assert bad.any(axis=1).mean() <= 1e-4, (bad.sum(), np.abs(gx - rx).max(), scale)
    return absP


@pytest.mark.gpu
def test_backward_default_config_random_and_surface_points():
    _check_backward(np.random.default_rng(2).uniform(-0.02, 1.02, (100_000, 3)).astype(np.float32), DEFAULT)
    _check_backward(_mario_points(), DEFAULT, seed=3)


@pytest.mark.gpu
@pytest.mark.parametrize("F", [1, 4, 8])
def test_backward_features_per_level(F):
    cfg = dict(DEFAULT, n_levels=6, n_features_per_level=F, log2_hashmap_size=14)
    _check_backward(np.random.default_rng(F).uniform(-0.05, 1.05, (40_000, 3)).astype(np.float32), cfg, seed=F)


@pytest.mark.gpu
def test_backward_contended_coarse_levels():
    """1 M points on coarse levels: level 0 (16^3 entries, the LDS path) takes ~2 000 adds per entry, level 1 (32^3, the global
    path) ~250; once in random order and once sorted, so that neighbouring lanes share entries (the on-chip run sums)."""
    cfg = {"otype": "HashGrid", "n_levels": 2, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16,
           "per_level_scale": 2.0}
    x = np.random.default_rng(4).uniform(0, 1, (1_000_000, 3)).astype(np.float32)
    absP = _check_backward(x, cfg, seed=5)
    assert absP[:4096 * 2].mean() > 100                               # (~2 000 adds of |w dy| ~ 0.1 per level-0 value)
    order = np.lexsort((x[:, 0], x[:, 1], x[:, 2]))
    _check_backward(np.ascontiguousarray(x[order]), cfg, seed=6)


@pytest.mark.gpu
def test_adjoint_identity_for_the_parameters():
    """The encoding is linear in the table: <dy, enc(x; dp)> == <J^T dy, dp> with J^T dy the backward's dL/dparams."""
    from tssplat_amd import encoding
    enc = encoding.GridEncoding(3, DEFAULT).cuda()
    x = torch.rand(500_000, 3, device="cuda") * 1.04 - 0.02
    dp = torch.rand_like(enc.params) * 2 - 1
    dy = torch.randn(500_000, 32, device="cuda")
    with torch.no_grad():
        enc.params.copy_(dp)
    lhs = (enc(x).double() * dy.double()).sum()
    enc.params.grad = None
    enc(x).backward(dy)
    rhs = (enc.params.grad.double() * dp.double()).sum()
    assert abs(float(lhs - rhs)) <= 1e-4 * float((enc(x).abs().double() * dy.abs().double()).sum()), (float(lhs), float(rhs))


@pytest.mark.gpu
def test_texture_stage_size_call():
    """120 x 512^2 points (31.5 M): the 64-bit point and output offsets (the output alone is 4 GB), finite results, and the
    last rows -- where an int32 offset would have wrapped -- equal to the oracle."""
    from tssplat_amd import encoding
    N = 120 * 512 * 512
    enc = encoding.GridEncoding(3, DEFAULT).cuda()
    with torch.no_grad():
        enc.params.uniform_(-1, 1)
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.rand(N, 3, device="cuda", generator=g).requires_grad_(True)
    y = enc(x)
    assert y.shape == (N, 32) and bool(torch.isfinite(y).all())
    tail = slice(N - 4096, N)
    lay = _lay(DEFAULT)
    P = enc.params.detach().cpu().numpy()
    xt = x.detach()[tail].cpu().numpy()
    assert np.abs(y.detach()[tail].cpu().double().numpy() - O.encode(xt, P, lay)).max() <= 4e-6
    dy = torch.zeros_like(y)
    dy[tail] = 1.0
    y.backward(dy)
    del y, dy
    assert bool(torch.isfinite(enc.params.grad).all()) and bool(torch.isfinite(x.grad).all())
    assert float(x.grad[: N - 4096].abs().max()) == 0.0
    _, rx = O.encode_backward(xt, P, np.ones((4096, 32)), lay)
    assert np.abs(x.grad[tail].cpu().double().numpy() - rx).max() <= 1e-3 * np.abs(rx).max()


def _texture_setup(optimize_geo, views=8, res=128):
    from tssplat_amd import geometry, materials, renderers, scenes
    m = np.load(os.path.join(ROOT, "tests", "golden", "mario_mesh.npz"))
    v, f = m["vertices"].astype(np.float32), m["faces"].astype(np.int32)
    geo = geometry.TetMeshGeometry(v, np.zeros((0, 4), np.int32), use_smooth_barrier=False, optimize_geo=optimize_geo,
                                   surface_vid=np.arange(v.shape[0], dtype=np.int32), surface_fid=f)
    mvp = torch.from_numpy(scenes.dataset_mvps(views).astype(np.float32)).cuda()
    bg = torch.ones(views, res, res, 3, device="cuda")

    class Field(torch.nn.Module):                                    # the known colour field the targets are rendered from
        def forward(self, positions):
            return {"color": 0.5 + 0.5 * torch.sin(torch.stack([3.0 * positions[..., 0] + 1.0, 4.0 * positions[..., 1],
                                                                 5.0 * positions[..., 2] - 0.5], -1))}
    with torch.no_grad():
        target = renderers.MeshRasterizer(geo, Field())(mvp, only_alpha=False, iter_num=0, resolution=res, background=bg)["shaded"]
    torch.manual_seed(0)
    mat = materials.ExplicitMaterial({"n_output_dims": 3, "material_activation": "sigmoid"})
    return geo, renderers.MeshRasterizer(geo, mat), mvp, bg, target.clone(), res


@pytest.mark.gpu
def test_texture_stage_fits_a_known_colour_field():
    """trainer.py:44-49,56,102-104: frozen geometry, L1 on RGB, AdamUniform (lr 0.05) over renderer.parameters(); 150 iterations take the
    loss below a quarter of its start."""
    from tssplat_amd.utils.optimizer import AdamUniform
    geo, ren, mvp, bg, target, res = _texture_setup(optimize_geo=False)
    assert not any(p is geo.tet_v for p in ren.parameters())
    opt = AdamUniform(ren.parameters(), lr=0.05)
    loss_fn = torch.nn.L1Loss()
    losses = []
    for it in range(150):
        out = ren(mvp, only_alpha=False, iter_num=it, resolution=res, background=bg)
        loss = loss_fn(out["shaded"][..., :3], target[..., :3]) * 20
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert np.isfinite(losses).all()
    assert losses[-1] < 0.25 * losses[0], (losses[0], losses[-1])


@pytest.mark.gpu
def test_colour_gradient_reaches_the_geometry():
    """optimize_geo: the colour loss reaches tet_v through the encoding's dL/dx (on top of the silhouette path of antialias)."""
    geo, ren, mvp, bg, target, res = _texture_setup(optimize_geo=True, views=4, res=96)

    def grad(detach_positions):
        mat = ren.materials
        fwd = mat.forward
        if detach_positions:
            mat.forward = lambda positions, **kw: fwd(positions.detach(), **kw)
        try:
            geo.tet_v.grad = None
            out = ren(mvp, only_alpha=False, iter_num=0, resolution=res, background=bg)
            torch.nn.L1Loss()(out["shaded"][..., :3], target[..., :3]).backward()
        finally:
            mat.forward = fwd
        return geo.tet_v.grad.clone()
    g = grad(False)
    enc = ren.materials.encoding.encoding.encoding
    assert enc.params.grad is not None and float(enc.params.grad.abs().max()) > 0
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    colour_part = g - grad(True)
    assert float(colour_part.abs().max()) > 1e-3 * float(g.abs().max())
