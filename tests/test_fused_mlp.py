"""Fully fused MLP (tssplat_amd.network / tcnn.Network / tcnn.NetworkWithInputEncoding / models, csrc/mlp_kernels.hip) against
the float64 oracle tests/mlp_oracle.py.

CPU tier: layout known answers, the C ABI's rejections, the config rejections, seeded construction, the oracle's own
consistency (finite differences, an nn.Linear chain) and the reference's unmodified modules building tcnn networks on the
stand-in; mlp_oracle.plan (the launch code's choice of kernel variant, pass split and LDS mode) pinned to the C ABI over the
whole envelope, with the proof that EXACT_CONFIGS reaches every launch class and that <16, 32> is unreachable; the
preconditions of the dense exact data.  GPU tier: bitwise known answers on exact dyadic data (the sparse generator on four
configs; the dense one on a member of every launch class at 1, 63, 257 rows and past the backward's workgroup cap), the
dx-only and dW-only calls bitwise against the joint call, the forward's persistent loop at 2048 * 64 + 65 rows and the
independence of a row from its neighbours, misaligned / strided / half / double x and an expanded dy, the Sigmoid output on
exact pre-activations to 2 ulp, random data against the rounding-emulating oracle, the adjoint identity, bitwise
repeatability, a call above 2^31 input bytes, NetworkWithInputEncoding = Encoding + Network, and the texture stage through the
renderer with a FullyFusedMLP colour network."""
import ctypes as C
import functools
import importlib
import os
import sys
import types

import numpy as np
import pytest
import torch

import mlp_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
ACT = {"relu": 1, "none": 0, "sigmoid": 2}
GRID = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16,
        "per_level_scale": 1.447269237440378}
# (n_in, n_out, width, hidden layers, activation, output activation): every width, L = 1 / 2 / 5 / 8, n_in 3 / 32 / 33 / 256,
# n_out 1 / 3 / 17 / 64, both activations of each kind; the last two need several dW passes
CONFIGS = [(32, 3, 64, 1, "relu", "none"), (32, 3, 64, 2, "relu", "sigmoid"), (33, 17, 16, 5, "none", "none"),
           (3, 1, 32, 2, "none", "sigmoid"), (256, 17, 32, 8, "relu", "none"), (33, 64, 16, 1, "relu", "sigmoid"),
           (3, 3, 128, 5, "relu", "none"), (256, 64, 128, 8, "relu", "sigmoid")]
# The configurations compared bitwise on dense exact data: one or more of every (width, dW slots per wave, multi-pass,
# forward resident, backward resident, backward LDS above 64 KiB) class that mlp_oracle.plan finds in the envelope
# (test_plan_table_... asserts that), and the edges of the slot rule.
EXACT_CONFIGS = [c for c in CONFIGS if c[5] == "none"] + [
    (1, 1, 128, 1, "relu", "none"),        # <128, 8>, 16 tiles, one real input and 15 bias columns
    (17, 17, 128, 1, "none", "none"),      # <128, 8>, exactly 32 tiles: every slot used; LDS above 64 KiB
    (32, 17, 64, 2, "relu", "none"),       # <64, 8>, exactly 32 tiles
    (33, 17, 64, 2, "relu", "none"),       # 36 tiles: the first <64, 32>
    (1, 64, 64, 2, "relu", "none"),        # <64, 32>, forward and backward resident
    (128, 1, 64, 3, "relu", "none"),       # forward resident, backward re-staging
    (33, 1, 64, 8, "relu", "none"),        # forward re-staging, one pass of exactly 128 tiles
    (128, 1, 64, 7, "relu", "none"),       # two passes, the second holding the output matrix alone
    (256, 1, 64, 5, "relu", "none"),       # two passes, LDS above 64 KiB
    (256, 64, 32, 8, "relu", "none"),      # <32, 32>, forward resident, backward re-staging
    (256, 1, 16, 1, "relu", "none"),       # <16, 8>, LDS above 64 KiB
    (17, 17, 32, 2, "relu", "none"),       # <32, 8>
    (128, 17, 32, 5, "relu", "none"),      # <32, 32>, resident, LDS below 64 KiB
    (256, 17, 64, 1, "relu", "none"),      # <64, 32>, one pass, backward re-staging, LDS above 64 KiB
    (128, 17, 64, 1, "relu", "none"),      # <64, 32>, one pass, backward resident, LDS above 64 KiB
    (128, 17, 128, 1, "relu", "none"),     # <128, 32>, one pass, backward re-staging
    (17, 64, 128, 1, "relu", "none"),      # <128, 32>, one pass, backward resident
    (256, 64, 128, 8, "relu", "none")]     # the largest network of the envelope: five passes
GRADIENT_PATH_CONFIGS = [(32, 3, 64, 1, "relu", "none"), (128, 1, 64, 7, "relu", "none"), (3, 3, 128, 5, "relu", "none"),
                         (256, 64, 32, 8, "relu", "none")]
SIGMOID_CONFIGS = [c[:5] + ("sigmoid",) for c in [CONFIGS[1], CONFIGS[3], CONFIGS[5], (128, 1, 64, 7, "relu"), CONFIGS[7]]]
FWD_MAX_BLOCKS = 2048                       # kFwdMaxBlocks of csrc/mlp_kernels.hip


def _stride_rows(conf):
    """The smallest ragged row count past the backward's workgroup cap: cap + 2 blocks of 64 rows, so workgroups 0 and 1
    take a second block, and the last block holds a single row."""
    return O.plan(*conf[:4])["cap"] * 64 + 65


def _net_cfg(width, hidden, act, out_act, otype="FullyFusedMLP"):
    return {"otype": otype, "n_neurons": width, "n_hidden_layers": hidden, "activation": {"relu": "ReLU", "none": "None"}[act],
            "output_activation": {"none": "None", "sigmoid": "Sigmoid"}[out_act]}


# ------------------------------------------------------------------------------------------------------------------ CPU tier
def test_layout_known_answers():
    from tssplat_amd import network
    for (n_in, n_out, W, L), (n, in_w, out_w) in [((32, 3, 64, 1), (3072, 32, 16)), ((3, 3, 128, 5), (69_632, 16, 16)),
                                                  ((33, 17, 16, 2), (1536, 48, 32))]:
        lay = network.mlp_layout(network.parse_mlp_config(n_in, n_out, {"n_neurons": W, "n_hidden_layers": L}))
        assert (lay["n_params"], lay["in_w"], lay["out_w"]) == (n, in_w, out_w)
        ol = O.layout(n_in, n_out, W, L)
        assert (ol["n_params"], ol["in_w"], ol["out_w"]) == (n, in_w, out_w) and ol["shapes"] == lay["shapes"]


def _envelope():
    for W in (16, 32, 64, 128):
        for L in range(1, 9):
            for n_in in (1, 16, 17, 32, 33, 64, 128, 256):
                for n_out in (1, 16, 17, 64):
                    yield n_in, n_out, W, L


def test_plan_table_matches_the_library_and_the_gpu_table_reaches_every_class(capsys):
    """mlp_oracle.plan against what the C ABI shows of the launch code (n_params, and the workgroup cap that follows from
    the slot class: 512 with 8 slots, 256 with 32) over the whole envelope; the pass split is well formed; <16, 32> cannot
    occur; and EXACT_CONFIGS, which test_dense_exact_known_answers_are_bitwise compares bitwise, holds a member of every
    (width, slots, multi-pass, forward resident, backward resident, backward LDS above 64 KiB) class of the envelope."""
    from tssplat_amd import _capi
    lib = _capi.load()
    classes = {}
    for n_in, n_out, W, L in _envelope():
        p, lay = O.plan(n_in, n_out, W, L), O.layout(n_in, n_out, W, L)
        n = C.c_int64(0)
        assert lib.tsamd_mlp_layout(n_in, n_out, W, L, 1, 0, C.byref(n), None, None) == 0 and n.value == lay["n_params"]
        ws = lib.tsamd_mlp_workspace_bytes(64 * 1000, n_in, n_out, W, L, 1, 0)
        assert ws == 4 * lay["n_params"] * p["cap"], (n_in, n_out, W, L, ws, p)
        assert p["cap"] == {8: 512, 32: 256}[p["slots"]]
        assert (W, p["slots"]) != (16, 32), (n_in, n_out, W, L)          # mlp_backward_kernel<16, 32> is unreachable
        assert p["passes"][0][0] == 0 and p["passes"][-1][1] == L
        for i, (lo, hi) in enumerate(p["passes"]):
            assert lo <= hi and 0 < sum(p["tiles"][lo:hi + 1]) <= 4 * p["slots"], (n_in, n_out, W, L, p["passes"])
            assert i == 0 or lo == p["passes"][i - 1][1] + 1
        assert p["slots"] == 32 or len(p["passes"]) == 1
        assert p["fwd_resident"] or not p["bwd_resident"]
        assert max(p["fwd_lds"], p["bwd_lds"]) <= 160 * 1024              # the LDS of a gfx950 compute unit
        classes.setdefault(p["cls"], []).append((n_in, n_out, W, L))
    # the edges the GPU table names: a width-128 network has 8 slots only with one hidden layer and in_w + out_w <= 64
    assert O.plan(16, 16, 128, 1)["slots"] == 8 and O.plan(17, 17, 128, 1)["slots"] == 8 and O.plan(33, 17, 128, 1)["slots"] == 32
    assert sum(O.plan(17, 17, 128, 1)["tiles"]) == 32 and sum(O.plan(32, 17, 64, 2)["tiles"]) == 32
    assert O.plan(33, 17, 64, 2)["slots"] == 32 and O.plan(33, 1, 64, 8)["passes"] == [(0, 8)]
    assert sum(O.plan(33, 1, 64, 8)["tiles"]) == 128 and O.plan(128, 1, 64, 7)["passes"] == [(0, 6), (7, 7)]
    assert O.plan(3, 3, 128, 5)["passes"] == [(0, 1), (2, 3), (4, 5)]
    reached = {}
    for conf in EXACT_CONFIGS:
        reached.setdefault(O.plan(*conf[:4])["cls"], []).append(conf[:4])
    with capsys.disabled():
        print("\n(width, slots, multi-pass, fwd resident, bwd resident, bwd LDS > 64 KiB): envelope members, reached by")
        for cls in sorted(classes):
            print(f"  {cls}: {len(classes[cls])}, {reached.get(cls)}")
    assert len(classes) == 19
    assert set(classes) <= set(reached), sorted(set(classes) - set(reached))


def test_dense_exact_data_meets_its_preconditions():
    """The data of the bitwise GPU tests is exact and dense at the row counts that run without a device in well under a
    second (the GPU tests recompute the same conditions at theirs).  One row cannot be dense; it is held to the exactness
    conditions alone."""
    for conf in EXACT_CONFIGS:
        n_in, n_out, W, L, act, out_act = conf
        for N in (1, 63, 257):
            ex = O.exact_preconditions(*O.dense_exact_data(n_in, n_out, W, L, N, 0), n_out, W, L, act, out_act, dense=N >= 63)
            if N == 257 and n_in == 256:
                assert ex["stats"]["dx_share"] >= 0.25, (conf, ex["stats"])   # two tiled permutations alone give 4-8 %
    for conf in [(32, 3, 64, 1, "relu", "none"), (256, 64, 32, 8, "relu", "none")]:
        n_in, n_out, W, L, act, out_act = conf
        N = _stride_rows(conf)
        assert N == {8: 32_833, 32: 16_449}[O.plan(n_in, n_out, W, L)["slots"]]
        O.exact_preconditions(*O.dense_exact_data(n_in, n_out, W, L, N, 0), n_out, W, L, act, out_act)
    for conf in SIGMOID_CONFIGS:
        _sigmoid_case(conf, 257)


def test_c_abi_rejections_without_a_gpu():
    from tssplat_amd import _capi
    lib = _capi.load()

    def fwd(x=8, n=10, p=16, n_in=32, n_out=3, W=64, L=1, act=1, out_act=0, y=16):
        return lib.tsamd_mlp_forward(x, n, p, n_in, n_out, W, L, act, out_act, y, None)

    for kw, msg in [(dict(W=48), b"n_neurons"), (dict(L=0), b"n_hidden_layers"), (dict(L=9), b"n_hidden_layers"),
                    (dict(n_in=0), b"n_input_dims"), (dict(n_in=257), b"n_input_dims"), (dict(n_out=65), b"n_output_dims"),
                    (dict(n_out=0), b"n_output_dims"), (dict(act=2), b"activation"), (dict(act=-1), b"activation"),
                    (dict(out_act=1), b"output_activation"), (dict(out_act=3), b"output_activation"), (dict(n=-1), b"n_rows"),
                    (dict(x=None), b"x_dev"), (dict(p=None), b"params_dev"), (dict(y=None), b"y_dev")]:
        assert fwd(**kw) == 1, kw
        assert msg in lib.tsamd_last_error(), (kw, lib.tsamd_last_error())
    cfg = (32, 3, 64, 1, 1, 0)
    assert lib.tsamd_mlp_backward(8, 10, 16, *cfg, None, 16, 16, 16, None) == 1 and b"grad_y_dev" in lib.tsamd_last_error()
    assert lib.tsamd_mlp_backward(8, 10, 16, *cfg, 16, 16, None, None, None) == 1 and b"workspace_dev" in lib.tsamd_last_error()
    assert lib.tsamd_mlp_backward(None, 10, 16, *cfg, 16, 16, None, 16, None) == 1 and b"x_dev" in lib.tsamd_last_error()
    assert lib.tsamd_mlp_workspace_bytes(10, 32, 3, 48, 1, 1, 0) == -1
    assert lib.tsamd_mlp_workspace_bytes(0, *cfg) == 0 and lib.tsamd_mlp_workspace_bytes(10, *cfg) > 0
    assert lib.tsamd_mlp_layout(32, 3, 64, 9, 1, 0, None, None, None) == 1
    n, iw, ow = C.c_int64(0), C.c_int32(0), C.c_int32(0)
    assert lib.tsamd_mlp_layout(*cfg, C.byref(n), C.byref(iw), C.byref(ow)) == 0 and (n.value, iw.value, ow.value) == (3072, 32, 16)
    # nothing to do: no launch, no device needed
    assert fwd(n=0, x=None, p=None, y=None) == 0
    assert lib.tsamd_mlp_backward(None, 0, None, *cfg, None, None, None, None, None) == 0


def test_config_rejections():
    from tssplat_amd import network, tcnn
    base = {"otype": "FullyFusedMLP", "n_neurons": 64, "n_hidden_layers": 1}
    for bad, n_in, n_out in [(dict(base, n_neurons=48), 32, 3), (dict(base, n_hidden_layers=0), 32, 3),
                             (dict(base, n_hidden_layers=9), 32, 3), (dict(base, activation="Tanh"), 32, 3),
                             (dict(base, output_activation="ReLU"), 32, 3), (base, 257, 3), (base, 0, 3), (base, 32, 65)]:
        with pytest.raises(ValueError):
            tcnn.Network(n_in, n_out, bad)
    for cls in (tcnn.Network, tcnn.NetworkWithInputEncoding):
        with pytest.raises(NotImplementedError, match="VanillaMLP"):
            cls(3, 3, {})
    with pytest.raises(NotImplementedError, match="VanillaMLP"):
        tcnn.Network(3, 3, {"otype": "VanillaMLP", "n_neurons": 64, "n_hidden_layers": 1})
    # the network config is checked before the (here empty, hence invalid) encoding config
    with pytest.raises(NotImplementedError, match="VanillaMLP"):
        tcnn.NetworkWithInputEncoding(3, 3, {}, {"otype": "SIREN"})
    with pytest.raises(ValueError):
        tcnn.NetworkWithInputEncoding(3, 3, {}, base)
    for otype in ("FullyFusedMLP", "CutlassMLP", "MLP", "fullyfusedmlp"):
        assert network.is_network_otype(otype)
    cfg = network.parse_mlp_config(3, 3, {"otype": "CutlassMLP"})
    assert (cfg["n_neurons"], cfg["n_hidden_layers"], cfg["activation"], cfg["output_activation"]) == (128, 5, 1, 0)


def test_network_builds_on_the_cpu():
    """Construction needs no device: xavier-uniform matrices over their padded shapes, seeded."""
    from tssplat_amd import tcnn
    cfg = {"otype": "FullyFusedMLP", "n_neurons": 64, "n_hidden_layers": 2}
    a, b, c = tcnn.Network(33, 3, cfg, seed=7), tcnn.Network(33, 3, cfg, seed=7), tcnn.Network(33, 3, cfg, seed=8)
    n = 64 * 48 + 64 * 64 + 16 * 64
    assert a.params.shape == (n,) and a.params.dtype == torch.float32
    assert torch.equal(a.params.detach(), b.params.detach()) and not torch.equal(a.params.detach(), c.params.detach())
    off = 0
    for rows, cols in [(64, 48), (64, 64), (16, 64)]:
        m = a.params.detach()[off:off + rows * cols]
        bound = float(np.sqrt(6.0 / (rows + cols)))
        assert float(m.abs().max()) <= bound and float(m.abs().max()) > 0.9 * bound
        off += rows * cols
    ne = tcnn.NetworkWithInputEncoding(3, 3, GRID, cfg, seed=7)
    assert ne.params.shape == (64 * 32 + 64 * 64 + 16 * 64 + 12_599_920,)
    assert ne.network_params.numel() == 64 * 32 + 64 * 64 + 16 * 64 and ne.encoding_params.numel() == 12_599_920
    assert ne.network_params.data_ptr() == ne.params.data_ptr()      # views of the one Parameter
    with pytest.raises(RuntimeError):
        a(torch.zeros(4, 33))                                         # no CPU fallback


def test_oracle_exact_mode_against_finite_differences():
    rng = np.random.default_rng(0)
    for n_in, n_out, W, L, act, out_act in [(5, 3, 16, 2, "relu", "sigmoid"), (17, 2, 32, 1, "none", "none")]:
        lay = O.layout(n_in, n_out, W, L)
        P = rng.normal(0, 0.4, lay["n_params"])
        x = rng.normal(0, 1, (4, n_in))
        dy = rng.normal(0, 1, (4, n_out))
        b = O.backward(x.astype(np.float32), P, dy, n_out, W, L, act, out_act, exact=True)
        xd = x.astype(np.float32).astype(np.float64)

        def loss(P_, x_):
            return float((O.forward(x_, P_, n_out, W, L, act, out_act, exact=True)["y"] * dy).sum())
        eps = 1e-6
        for i in rng.choice(lay["n_params"], 40, replace=False):
            e = np.zeros_like(P)
            e[i] = eps
            fd = (loss(P + e, xd) - loss(P - e, xd)) / (2 * eps)
            assert abs(fd - b["dparams"][i]) <= 1e-5 * (1 + abs(fd)), (i, fd, b["dparams"][i])
        for r, k in [(0, 0), (1, n_in - 1), (3, n_in // 2)]:
            e = np.zeros_like(xd)
            e[r, k] = eps
            fd = (loss(P, xd + e) - loss(P, xd - e)) / (2 * eps)
            assert abs(fd - b["dx"][r, k]) <= 1e-5 * (1 + abs(fd))


def test_oracle_exact_forward_is_a_linear_chain_with_a_ones_column():
    rng = np.random.default_rng(1)
    n_in, n_out, W, L = 7, 5, 32, 3
    lay = O.layout(n_in, n_out, W, L)
    P = rng.normal(0, 0.3, lay["n_params"])
    x = rng.normal(0, 1, (9, n_in)).astype(np.float32)
    mats = [torch.from_numpy(m) for m in O.split(P, lay)]
    xin = torch.cat([torch.from_numpy(x).double(), torch.ones(9, lay["in_w"] - n_in, dtype=torch.float64)], 1)
    layers = []
    for m in mats:
        lin = torch.nn.Linear(m.shape[1], m.shape[0], bias=False).double()
        lin.weight.data.copy_(m)
        layers += [lin, torch.nn.ReLU()]
    seq = torch.nn.Sequential(*layers[:-1])
    ref = seq(xin)[:, :n_out].detach().numpy()
    assert np.allclose(O.forward(x, P, n_out, W, L, "relu", "none", exact=True)["y"], ref, rtol=1e-12, atol=1e-12)


@pytest.mark.skipif(not os.path.exists(os.path.join(REF, "models", "networks.py")),
                    reason="the reference checkout only exists in the authoring container")
def test_reference_networks_build_on_the_stand_in(monkeypatch):
    """The reference's unmodified models/networks.py and materials/explicit_material.py, with `tinycudann` bound to
    tssplat_amd.tcnn and omegaconf stubbed, torch.cuda.device patched out: its tcnn network routes build."""
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
        nets = importlib.import_module("models.networks")
        assert nets.__file__.startswith(REF)
        mlp_cfg = {"otype": "FullyFusedMLP", "n_neurons": 64, "n_hidden_layers": 1}
        net = nets.get_mlp(32, 3, _Node(mlp_cfg))
        assert isinstance(net, nets.TCNNNetwork) and isinstance(net.network, tcnn.Network)
        assert sum(p.numel() for p in net.parameters()) == 3072
        ne = nets.create_network_with_input_encoding(3, 3, _Node(GRID), _Node(mlp_cfg))
        assert isinstance(ne, nets.TCNNNetworkWithInputEncoding)
        assert sum(p.numel() for p in ne.parameters()) == 12_599_920 + 3072
        mat_mod = importlib.import_module("materials.explicit_material")
        monkeypatch.setattr(mat_mod, "get_device", lambda: torch.device("cpu"))
        m = mat_mod.ExplicitMaterial({"n_output_dims": 3, "material_activation": "sigmoid", "mlp_network_config": mlp_cfg})
        assert isinstance(m.feature_network, nets.TCNNNetwork)
        assert sum(p.numel() for p in m.feature_network.parameters()) == 3072
    finally:
        for name in [n for n in sys.modules if n.split(".")[0] in ("models", "materials", "utils")]:
            del sys.modules[name]


# ------------------------------------------------------------------------------------------------------------------ GPU tier
def _run(x_np, P_np, conf, dy_np=None, want_x=True, want_p=True):
    """(y, dL/dparams, dL/dx) of the HIP network as numpy float64."""
    from tssplat_amd import tcnn
    n_in, n_out, W, L, act, out_act = conf
    net = tcnn.Network(n_in, n_out, _net_cfg(W, L, act, out_act)).cuda()
    with torch.no_grad():
        net.params.copy_(torch.from_numpy(np.asarray(P_np, np.float32)))
    net.params.requires_grad_(want_p)
    x = torch.from_numpy(np.asarray(x_np, np.float32)).cuda().requires_grad_(want_x)
    y = net(x)
    assert y.dtype == torch.float32 and tuple(y.shape) == (x.shape[0], n_out)
    if dy_np is None:
        return y.detach().cpu().double().numpy(), None, None
    y.backward(torch.from_numpy(np.asarray(dy_np, np.float32)).cuda())
    gp = net.params.grad.cpu().double().numpy() if want_p else None
    gx = x.grad.cpu().double().numpy() if want_x else None
    return y.detach().cpu().double().numpy(), gp, gx


def _exact_data(conf, N, seed):
    """Integer inputs in [-2, 2], weights with at most two entries per row and two per column of every square block (two
    random permutations, one entry +1 so that ReLU networks stay alive, the other +-1), dy = k / 128 with |k| <= 2: every fp16 value is a small integer and every fp32 sum of integers stays
    far below 2^24, so the fp16 / fp32 arithmetic of the kernels is exact (checked against the oracle's exact mode below)."""
    n_in, n_out, W, L, act, out_act = conf
    rng = np.random.default_rng(seed)
    lay = O.layout(n_in, n_out, W, L)
    parts = []
    for rows, cols in lay["shapes"]:
        m = np.zeros((rows, cols))
        big = max(rows, cols)
        for sign, perm in enumerate((rng.permutation(big), rng.permutation(big))):
            keep = rng.random(rows) < 0.6
            m[np.arange(rows)[keep], perm[:rows][keep] % cols] += rng.choice([-1.0, 1.0], keep.sum()) if sign else 1.0
        parts.append(m.ravel())
    P = np.concatenate(parts)
    x = rng.integers(-2, 3, (N, n_in)).astype(np.float64)
    dy = rng.integers(-2, 3, (N, n_out)) / 128.0
    return x, P, dy


@pytest.mark.gpu
@pytest.mark.parametrize("conf", [c for c in CONFIGS if c[5] == "none"])
def test_exact_known_answers_are_bitwise(conf):
    """Forward, dx and dW bitwise equal to the oracle on exact data: catches any wrong MFMA lane map or operand order."""
    for N, seed in [(1, 0), (255, 1), (257, 2)]:
        x, P, dy = _exact_data(conf, N, seed)
        n_in, n_out, W, L, act, out_act = conf
        ex = O.backward(x, P, dy, n_out, W, L, act, out_act, exact=True)
        rd = O.backward(x, P, dy, n_out, W, L, act, out_act, exact=False)
        assert np.array_equal(ex["f"]["y"], rd["f"]["y"]) and np.array_equal(ex["dparams"], rd["dparams"])   # data is exact
        assert max(float(np.abs(a).max()) for a in ex["f"]["a"] + ex["deltas"]) <= 2048
        y, gp, gx = _run(x, P, conf, dy)
        assert np.array_equal(y, ex["f"]["y"]), np.abs(y - ex["f"]["y"]).max()
        assert np.array_equal(gx, ex["dx"]), np.abs(gx - ex["dx"]).max()
        assert np.array_equal(gp, ex["dparams"]), np.abs(gp - ex["dparams"]).max()


def _random_data(conf, N, seed):
    """Uniform x in [-1, 1], xavier-uniform matrices over their padded shapes, normal dy."""
    n_in, n_out, W, L, act, out_act = conf
    rng = np.random.default_rng(seed)
    lay = O.layout(n_in, n_out, W, L)
    P = np.concatenate([rng.uniform(-1, 1, r * c) * np.sqrt(6.0 / (r + c)) for r, c in lay["shapes"]])
    x = rng.uniform(-1, 1, (N, n_in)).astype(np.float32)
    dy = rng.normal(0, 1, (N, n_out)).astype(np.float32)
    return x, P, dy


@functools.lru_cache(maxsize=4)
def _dense_case(conf, N):
    """(x, params, dy, {y, dx, dparams}) of mlp_oracle.dense_exact_data with its preconditions asserted; computed once for
    the tests that share it.  One row cannot be dense and is held to the exactness conditions alone."""
    n_in, n_out, W, L, act, out_act = conf
    x, P, dy = O.dense_exact_data(n_in, n_out, W, L, N, 0)
    ex = O.exact_preconditions(x, P, dy, n_out, W, L, act, out_act, dense=N >= 63)
    return x, P, dy, {"y": ex["f"]["y"], "dx": ex["dx"], "dparams": ex["dparams"]}


def _rows(conf, rows):
    return _stride_rows(conf) if rows == "stride" else int(rows)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [1, 63, 257, "stride"])
@pytest.mark.parametrize("conf", EXACT_CONFIGS, ids=lambda c: "-".join(map(str, c[:5])))
def test_dense_exact_known_answers_are_bitwise(conf, rows):
    """y, dx and dW bitwise equal to the oracle on data where no 16 x 16 dW tile is empty, for a member of every launch class
    (test_plan_table_...) at one row, a partial block, a ragged block count and the backward's grid-stride loop: a dW tile
    written to the wrong slot, matrix or pass offset, or a block skipped or taken twice, changes non-zero values."""
    x, P, dy, ref = _dense_case(conf, _rows(conf, rows))
    y, gp, gx = _run(x, P, conf, dy)
    assert np.array_equal(y, ref["y"]), np.abs(y - ref["y"]).max()
    assert np.array_equal(gx, ref["dx"]), np.abs(gx - ref["dx"]).max()
    assert np.array_equal(gp, ref["dparams"]), (np.abs(gp - ref["dparams"]).max(), int((gp != ref["dparams"]).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [257, "stride"])
@pytest.mark.parametrize("data", ["exact", "random"])
@pytest.mark.parametrize("conf", GRADIENT_PATH_CONFIGS, ids=lambda c: "-".join(map(str, c[:5])))
def test_gradient_paths_alone_are_bitwise_the_joint_call(conf, data, rows):
    """dx from a dx-only call (grad_params NULL: one pass with no dW group and no workspace) and dW from dW-only calls
    (every pass stops at its lowest matrix; W_0's transpose is never staged) are bitwise those of the call that wants both:
    the per-row arithmetic, the workgroup count and the partial-sum order do not depend on which outputs are asked for.  On
    the exact data all of them are the oracle's as well."""
    N = _rows(conf, rows)
    x, P, dy, ref = _dense_case(conf, N) if data == "exact" else _random_data(conf, N, 12) + (None,)
    y, gp, gx = _run(x, P, conf, dy)
    y_x, none_p, gx_only = _run(x, P, conf, dy, want_p=False)
    y_p, gp_only, none_x = _run(x, P, conf, dy, want_x=False)
    assert none_p is None and none_x is None and np.any(gx != 0) and np.any(gp != 0)
    assert np.array_equal(y_x, y) and np.array_equal(y_p, y)
    assert np.array_equal(gx_only, gx), np.abs(gx_only - gx).max()
    assert np.array_equal(gp_only, gp), np.abs(gp_only - gp).max()
    if ref is not None:
        assert np.array_equal(y, ref["y"]) and np.array_equal(gx_only, ref["dx"]) and np.array_equal(gp_only, ref["dparams"])


@pytest.mark.gpu
@pytest.mark.parametrize("conf", [(32, 3, 64, 2, "relu", "none"), (3, 3, 128, 5, "relu", "none"), (33, 1, 64, 8, "relu", "none")],
                         ids=lambda c: "-".join(map(str, c[:5])))
def test_forward_persistent_loop_and_row_independence(conf):
    """2048 * 64 + 65 rows: workgroups 0 and 1 of the forward's 2048 take a second block (`blk += gridDim.x`), in the resident
    mode and in the re-staging mode, whose image() synchronises the workgroup inside that loop.  y is bitwise the oracle's on
    dense exact data (forward only: the dW mass of this many rows would pass 2^24).  On random data y and dx of the first 257
    and of the last 321 rows, each computed in a call of their own, are bitwise those rows of the big call."""
    n_in, n_out, W, L, act, out_act = conf
    N = FWD_MAX_BLOCKS * 64 + 65
    assert O.plan(n_in, n_out, W, L)["fwd_resident"] == (conf[:4] == (32, 3, 64, 2))
    x, P, _ = O.dense_exact_data(n_in, n_out, W, L, N, 0)
    ex = O.forward(x, P, n_out, W, L, act, out_act, exact=True)
    assert np.array_equal(ex["y"], O.forward(x, P, n_out, W, L, act, out_act, exact=False)["y"])      # the data is exact
    assert max(float(np.abs(a).max()) for a in ex["a"]) <= 2048 and float(np.abs(ex["y"]).max()) < 2.0 ** 24
    ref = ex["y"]
    del ex
    y, _, _ = _run(x, P, conf)
    assert np.array_equal(y, ref), (np.abs(y - ref).max(), np.flatnonzero(np.any(y != ref, axis=1))[:8])
    x, P, dy = _random_data(conf, N, 13)
    y, _, gx = _run(x, P, conf, dy, want_p=False)
    for part in (slice(0, 257), slice(N - 321, N)):
        y_part, _, gx_part = _run(x[part], P, conf, dy[part], want_p=False)
        assert np.array_equal(y_part, y[part]) and np.array_equal(gx_part, gx[part]), part


def _net(conf, P_np):
    from tssplat_amd import tcnn
    n_in, n_out, W, L, act, out_act = conf
    net = tcnn.Network(n_in, n_out, _net_cfg(W, L, act, out_act)).cuda()
    with torch.no_grad():
        net.params.copy_(torch.from_numpy(np.asarray(P_np, np.float32)))
    return net


def _grads(net, x, dy=None):
    """(y, dL/dparams, dL/dx) for x as given (its dtype, strides and storage offset kept); dy None: y.sum().backward()."""
    net.params.grad = None
    x = x.detach().requires_grad_(True)
    y = net(x)
    if dy is None:
        y.sum().backward()
    else:
        y.backward(dy)
    return y.detach().cpu(), net.params.grad.cpu().clone(), x.grad.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("conf", [(32, 3, 64, 1, "relu", "none"), (256, 1, 16, 1, "relu", "none")], ids=lambda c: "-".join(map(str, c[:5])))
def test_input_forms_the_binding_accepts(conf):
    """x that is contiguous but only 4-byte aligned (load_x's scalar path where n_in % 4 == 0 normally takes float4 loads),
    strided x, half and double x, and the expanded dy of y.sum().backward(): bitwise the results of the plain call."""
    n_in, n_out, W, L, act, out_act = conf
    N = 257
    x_np, P, dy_np = _random_data(conf, N, 14)
    net = _net(conf, P)
    x, dy = torch.from_numpy(x_np).cuda(), torch.from_numpy(dy_np).cuda()
    assert x.data_ptr() % 16 == 0
    plain = _grads(net, x, dy)
    assert all(bool(t.abs().max() > 0) for t in plain)

    buf = torch.zeros(N * n_in + 8, device="cuda")
    shifted = buf[1:1 + N * n_in].view(N, n_in)
    shifted.copy_(x)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4
    for got, want in zip(_grads(net, shifted, dy), plain):
        assert torch.equal(got, want)

    wide = torch.zeros(N, 2 * n_in, device="cuda")
    wide[:, ::2] = x
    transposed = x.t().contiguous().t()
    assert not wide[:, ::2].is_contiguous() and not transposed.is_contiguous()
    for view in (wide[:, ::2], transposed):
        for got, want in zip(_grads(net, view, dy), plain):
            assert torch.equal(got, want)

    for dtype in (torch.float16, torch.float64):
        cast = x.half() if dtype == torch.float16 else x.double() * (1.0 + 2.0 ** -30)   # a double that float32 must round
        want = _grads(net, cast.float(), dy)
        got = _grads(net, cast, dy)
        assert got[2].dtype == dtype
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2].to(dtype))

    for got, want in zip(_grads(net, x), _grads(net, x, torch.ones(N, n_out, device="cuda"))):
        assert torch.equal(got, want)


def _sigmoid_case(conf, N, boost=1.0):
    """Dense exact data whose output matrix is scaled by the largest 2^-k that puts the median |z| below 8: (x, params,
    float64 y, z).  The scaled weights are fp16 values and every z is a small integer times 2^-k, so the kernel's fp32 z is
    exact and its y differs from the float64 sigmoid only by the float32 chain exponential, add, divide.  ``boost`` (a power
    of two) scales the output matrix further, into the range where the exponential leaves the float range."""
    n_in, n_out, W, L, act, out_act = conf
    assert out_act == "sigmoid"
    x, P, _ = O.dense_exact_data(n_in, n_out, W, L, N, 0)
    median = float(np.median(np.abs(O.forward(x, P, n_out, W, L, act, "none", exact=True)["y"])))
    k = 0
    while median * 2.0 ** -k >= 8.0:
        k += 1
    assert k <= 14                                                          # 2^-14: the smallest normal fp16
    x, P, _ = O.dense_exact_data(n_in, n_out, W, L, N, 0, out_scale=2.0 ** -k * boost)
    ex = O.forward(x, P, n_out, W, L, act, out_act, exact=True)
    rd = O.forward(x, P, n_out, W, L, act, out_act, exact=False)
    assert np.array_equal(ex["z"], rd["z"]) and max(float(np.abs(a).max()) for a in ex["a"]) <= 2048
    z = ex["z"][:, :n_out]
    assert float(np.abs(z).max()) * 2.0 ** k < 2.0 ** 24 and np.array_equal(z, z.astype(np.float32))
    assert np.mean(np.abs(z) < 8.0) >= 0.5 or boost > 1.0
    return x, P, ex["y"], z


@pytest.mark.gpu
@pytest.mark.parametrize("conf", SIGMOID_CONFIGS, ids=lambda c: "-".join(map(str, c[:5])))
def test_sigmoid_output_on_exact_pre_activations(conf):
    """The Sigmoid output on pre-activations the kernel computes exactly, at least half of them with |z| < 8 and the rest
    reaching |z| = 18 .. 40.  Derived bound: 2 ulp of float32 relative to y (1 ulp for the exponential -- exp2f's documented
    error plus 0.2 ulp of argument reduction, csrc/mlp_kernels.hip exp_by_fma --, 1/2 each for the add and the divide, and
    1 / (1 + e) amplifies a relative error of e by at most 1); 2^-126 covers results below the normal range.
    Observed on an MI355X: at most 0.83 ulp over the five configurations (0.47 .. 0.83), which is why the derived 2 ulp is
    asserted and not a wider 4.  With expf in the kernel the same data gave 7.2 ulp at z = -28."""
    x, P, ref, z = _sigmoid_case(conf, 4161)
    y, _, _ = _run(x, P, conf)
    err = np.abs(y - ref)
    ulps = float((err / (2.0 ** -23 * ref))[ref > 2.0 ** -100].max())
    print(f"sigmoid {conf[:5]}: max |y - ref| = {ulps:.3f} ulp relative, {float(np.mean(np.abs(z) < 8.0)):.2f} of |z| < 8, "
          f"max |z| = {float(np.abs(z).max()):.1f}")
    assert np.all(err <= 2.0 * 2.0 ** -23 * ref + 2.0 ** -126), ulps
    # the same bound where e^-z overflows (y = 0) or vanishes (y = 1): z reaches +-288 .. +-640
    x, P, ref, z = _sigmoid_case(conf, 257, boost=16.0)
    assert float(z.max()) > 104 and (float(z.min()) < -104 or conf[1] == 1)     # one output: one sign pattern, -36 and -96
    y, _, _ = _run(x, P, conf)
    assert np.all(np.abs(y - ref) <= 2.0 * 2.0 ** -23 * ref + 2.0 ** -126)
    assert np.all(y[z >= 20] == 1.0) and np.all(y[z < -104] == 0.0)


def _rows_within(err, s, N, what):
    """All but 2 % of the rows (at least eight may miss) within 2^-8 s + 1e-6."""
    assert np.all(np.isfinite(err)), what
    bad = np.any(err > 2.0 ** -8 * s + 1e-6, axis=1)
    assert bad.sum() <= max(8, N // 50), (what, int(bad.sum()), err.max())


def _bounds_check(conf, N, seed):
    """Random data against the rounding-emulating oracle.  The kernel and the oracle round the same values to fp16, but the
    kernel sums in fp32 where the oracle sums in float64, so a stored fp16 activation or delta may land one fp16 ulp
    (2^-11 relative) away.  Bound: 2^-8 of the last sum's absolute mass, s = sum |W_out| |a_L| (y; times 1/4 under Sigmoid),
    sum |W_1| |delta_1| / S (dx), sum over rows |delta| |a| / S (dW), plus 1e-6 for results near zero.  In a deep network an
    early flip (an fp16 rounding, or a ReLU mask whose pre-activation lies within an fp32 rounding of zero) is carried
    through every later layer; a flipped mask even gates a whole delta that the oracle's s does not count.  A numpy restatement
    of these semantics that sums in float32 misses this bound on 0.37 % of the dx rows of the 256 -> 32 x 8 -> 17 ReLU network
    at 100 003 rows (the kernel on 0.36 %, nearly the same rows), so 1 % of the y and dx rows may miss it; dW sums over all rows, which dilutes a single row, and must meet 2^-8 everywhere."""
    n_in, n_out, W, L, act, out_act = conf
    x, P, dy = _random_data(conf, N, seed)
    lay = O.layout(n_in, n_out, W, L)
    y, gp, gx = _run(x, P, conf, dy)
    ref = O.backward(x, P, dy, n_out, W, L, act, out_act)
    f = ref["f"]
    s_y = (np.abs(f["a"][-1]) @ np.abs(f["mats"][-1]).T)[:, :n_out]
    if out_act == "sigmoid":
        s_y = s_y * 0.25                                               # sigmoid' <= 1/4
    _rows_within(np.abs(y - f["y"]), s_y, N, "y")
    s_dx = (np.abs(ref["deltas"][0]) @ np.abs(f["mats"][0]))[:, :n_in] / O.LOSS_SCALE
    _rows_within(np.abs(gx - ref["dx"]), s_dx, N, "dx")
    s_dw = np.concatenate([(np.abs(ref["deltas"][m]).T @ np.abs(f["a"][m])).ravel() for m in range(L + 1)]) / O.LOSS_SCALE
    miss = np.abs(gp - ref["dparams"]) > 2.0 ** -8 * s_dw + 1e-6
    assert miss.sum() <= max(1, gp.size // 10), (int(miss.sum()), np.abs(gp - ref["dparams"]).max())
    off = 0
    for r, c in lay["shapes"]:
        k, o = gp[off:off + r * c], ref["dparams"][off:off + r * c]
        off += r * c
        assert np.linalg.norm(k - o) <= 3e-2 * np.linalg.norm(o) + 1e-6, (r, c, np.linalg.norm(k - o) / np.linalg.norm(o))
    return y, gp, gx


@pytest.mark.gpu
@pytest.mark.parametrize("conf", CONFIGS)
def test_random_data_against_the_oracle(conf):
    for N, seed in [(1, 3), (257, 4), (100_003, 5)]:
        _bounds_check(conf, N, seed)


@pytest.mark.gpu
def test_zero_rows():
    from tssplat_amd import tcnn
    net = tcnn.Network(32, 3, _net_cfg(64, 1, "relu", "none")).cuda()
    x = torch.zeros(0, 32, device="cuda", requires_grad=True)
    y = net(x)
    assert tuple(y.shape) == (0, 3)
    y.sum().backward()
    assert float(net.params.grad.abs().max()) == 0.0 and tuple(x.grad.shape) == (0, 32)


@pytest.mark.gpu
@pytest.mark.parametrize("conf", [(32, 3, 64, 1, "none", "none"), (33, 17, 16, 2, "none", "sigmoid")])
def test_adjoint_identity(conf):
    """<dy, J dp> = <J^T dy, dp> for the parameters and <dy, J dx> = <J^T dy, dx> for x, J by central differences of the
    kernel's own forward.  Without ReLU the network is smooth (multilinear up to the output Sigmoid), so the central
    difference has no kink error; fp16 rounding of the activations leaves noise of ~2^-11 / (2 eps) per element."""
    from tssplat_amd import tcnn
    n_in, n_out, W, L, act, out_act = conf
    rng = np.random.default_rng(6)
    net = tcnn.Network(n_in, n_out, _net_cfg(W, L, act, out_act), seed=3).cuda()
    x = torch.from_numpy(rng.uniform(-1, 1, (4096, n_in)).astype(np.float32)).cuda().requires_grad_(True)
    dy = torch.from_numpy(rng.normal(0, 1, (4096, n_out)).astype(np.float32)).cuda()
    net(x).backward(dy)
    dp = torch.from_numpy(rng.normal(0, 1, net.params.numel()).astype(np.float32)).cuda()
    dxv = torch.from_numpy(rng.normal(0, 1, (4096, n_in)).astype(np.float32)).cuda()
    with torch.no_grad():
        p0 = net.params.detach().clone()
        eps = 1e-2
        net.params.copy_(p0 + eps * dp)
        yp = net(x.detach())
        net.params.copy_(p0 - eps * dp)
        ym = net(x.detach())
        net.params.copy_(p0)
        lhs = float(((yp - ym) / (2 * eps) * dy).double().sum())
        rhs = float((net.params.grad * dp).double().sum())
        assert abs(lhs - rhs) <= 2e-2 * abs(rhs) + 1e-3, (lhs, rhs)
        yp, ym = net(x.detach() + eps * dxv), net(x.detach() - eps * dxv)
        lhs = float(((yp - ym) / (2 * eps) * dy).double().sum())
        rhs = float((x.grad * dxv).double().sum())
        assert abs(lhs - rhs) <= 2e-2 * abs(rhs) + 1e-3, (lhs, rhs)


@pytest.mark.gpu
@pytest.mark.parametrize("conf", [CONFIGS[0], CONFIGS[7]])
def test_bitwise_repeatable_and_rows_independent_of_n(conf):
    n_in, n_out, W, L, act, out_act = conf
    rng = np.random.default_rng(7)
    lay = O.layout(n_in, n_out, W, L)
    P = rng.uniform(-0.3, 0.3, lay["n_params"])
    x = rng.uniform(-1, 1, (100_003, n_in)).astype(np.float32)
    dy = rng.normal(0, 1, (100_003, n_out)).astype(np.float32)
    a = _run(x, P, conf, dy)
    b = _run(x, P, conf, dy)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    y_small, _, _ = _run(x[:257], P, conf)
    assert np.array_equal(y_small, a[0][:257])


@pytest.mark.gpu
def test_call_above_two_gigabytes_of_input():
    """17 M rows x 32 inputs (2.2 GB of x, 64-bit row offsets): finite everywhere, spot rows against the oracle."""
    from tssplat_amd import tcnn
    conf = (32, 3, 64, 1, "relu", "none")
    N = 17_000_000
    net = tcnn.Network(32, 3, _net_cfg(64, 1, "relu", "none"), seed=11).cuda()
    x = torch.rand(N, 32, device="cuda", generator=torch.Generator("cuda").manual_seed(0)) * 2 - 1
    x.requires_grad_(True)
    assert x.numel() * 4 > 2 ** 31
    y = net(x)
    dy = torch.ones_like(y)
    y.backward(dy)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(x.grad).all()) and bool(torch.isfinite(net.params.grad).all())
    rows = torch.tensor([0, 1, N // 2, N - 2, N - 1, 2 ** 31 // 128 + 5], device="cuda")
    xs = x.detach()[rows].cpu().numpy()
    P = net.params.detach().cpu().numpy()
    ref = O.backward(xs, P, np.ones((len(rows), 3)), 3, 64, 1)
    f = ref["f"]
    s_y = np.abs(f["a"][-1]) @ np.abs(f["mats"][-1]).T
    assert np.all(np.abs(y.detach()[rows].cpu().double().numpy() - f["y"]) <= 2.0 ** -8 * s_y[:, :3] + 1e-6)
    s_dx = (np.abs(ref["deltas"][0]) @ np.abs(f["mats"][0]))[:, :32] / O.LOSS_SCALE
    assert np.all(np.abs(x.grad[rows].cpu().double().numpy() - ref["dx"]) <= 2.0 ** -8 * s_dx + 1e-6)
    del conf


@pytest.mark.gpu
def test_network_with_input_encoding_equals_encoding_then_network():
    from tssplat_amd import tcnn
    cfg = _net_cfg(64, 1, "relu", "none")
    ne = tcnn.NetworkWithInputEncoding(3, 3, GRID, cfg, seed=5).cuda()
    enc, net = tcnn.Encoding(3, GRID).cuda(), tcnn.Network(32, 3, cfg).cuda()
    with torch.no_grad():
        enc.params.copy_(ne.encoding_params)
        net.params.copy_(ne.network_params)
    x = torch.rand(20_000, 3, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    dy = torch.randn(20_000, 3, device="cuda", generator=torch.Generator("cuda").manual_seed(2))
    y1 = ne(x)
    y2 = net(enc(x))
    assert torch.equal(y1, y2)
    y1.backward(dy)
    y2.backward(dy)
    g = ne.params.grad
    gn, ge = g[: ne.n_network_params], g[ne.n_network_params:]
    assert torch.equal(gn, net.params.grad)
    assert float(gn.abs().max()) > 0 and float(ge.abs().max()) > 0
    # the encoding's dL/dparams is a float-atomic sum (not bitwise repeatable): compare to a tolerance
    assert torch.allclose(ge, enc.params.grad, rtol=1e-4, atol=1e-7)


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
    mat = materials.ExplicitMaterial({"n_output_dims": 3, "material_activation": "sigmoid",
                                      "mlp_network_config": {"otype": "FullyFusedMLP", "activation": "ReLU",
                                                             "output_activation": "none", "n_neurons": 64, "n_hidden_layers": 1}})
    return geo, renderers.MeshRasterizer(geo, mat), mvp, bg, target.clone(), res


@pytest.mark.gpu
def test_texture_stage_fits_with_a_fully_fused_mlp():
    """The texture fit of test_hashgrid.py with mlp_network_config.otype = FullyFusedMLP: 150 iterations take the L1 loss
    below a quarter of its start."""
    from tssplat_amd import models
    from tssplat_amd.utils.optimizer import AdamUniform
    geo, ren, mvp, bg, target, res = _texture_setup(optimize_geo=False)
    assert isinstance(ren.materials.feature_network, models.TCNNNetwork)
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
def test_colour_gradient_reaches_the_geometry_through_the_fused_mlp():
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
    assert ren.materials.feature_network.network.params.grad is not None
    assert float(ren.materials.feature_network.network.params.grad.abs().max()) > 0
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    colour_part = g - grad(True)
    assert float(colour_part.abs().max()) > 1e-3 * float(g.abs().max())
