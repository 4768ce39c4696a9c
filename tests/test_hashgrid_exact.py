"""The hash-grid encoding (csrc/grid_kernels.hip, tssplat_amd/encoding.py) against the float64 oracle tests/hashgrid_oracle.py,
BIT FOR BIT: the forward, dL/dparams by the atomic, the sorted and the planned route, and dL/dx, on data on which every float32
operation is exact (tests/hashgrid_exact_data.py), at every launch edge of the kernels and on both sides of the LDS / global
split of the atomic route; the contracts of csrc/grid.h read through the C ABI (the backwards ADD, grad_x == NULL and
grad_params == NULL are launch paths of their own); derived rounding bounds on random data that hold for every element and
every point; and what can be pinned about inputs outside the defined domain.

CPU tier: the exactness conditions of the data (asserted from the oracle, not trusted), the expected LDS / global splits, the
deepest config the layout accepts, the tiling identity the 4 M-point case rests on.  GPU tier: everything else.  No tolerance
appears outside the random-data section."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import hashgrid_exact_data as D
import hashgrid_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGES = [1, 63, 64, 65,              # below, at and above one wave (segment_sums with invalid lanes)
         255, 256, 257,              # the 256-thread workgroup of the forward, dL/dx and the global atomic kernel
         1023, 1025,                 # the LDS kernel's 1024-thread workgroup
         4099,                       # the sorted route's tile tail
         16384, 16385]               # one LDS workgroup against two (ceil(N / 16384) of them)
ORDERS = ("random", "lexsorted")
# config A: entries 64, 512, 4096, 16384, 16384.  F moves the 128 KB LDS limit across the levels:
#   F = 1: level 3 and 4 are 64 KB exactly (the largest table launched without raising the dynamic-LDS attribute), all in LDS
#   F = 2: level 3 and 4 are 128 KB exactly: hashed levels in LDS, at the limit
#   F = 4: level 2 is 64 KB, levels 3 and 4 (256 KB) go to the global atomic kernel
#   F = 8: level 2 is 128 KB exactly, levels 3 and 4 global
LDS_SPLIT_A = {1: 5, 2: 5, 4: 3, 8: 3}
LDS_SPLIT_B = 3                      # DenseGrid, F = 2: 1 KB, 8 KB, 64 KB in LDS; 512 KB global
SECOND_TRIP_N = 256 * 16384 + 65     # past the LDS kernel's cap of 256 workgroups x 16 trips of its grid-stride loop
SECOND_TRIP_BASE = 4099


def _a(F):
    return dict(D.CONFIG_A, n_features_per_level=F)


def _log2(v):
    return float(np.log2(max(v, 1e-300)))


# ------------------------------------------------------------------------------------------------------------------ CPU tier
CONDITION_CASES = [("A-F1", _a(1), "scattered", {}), ("A-F2", _a(2), "scattered", {}), ("A-F4", _a(4), "scattered", {}),
                   ("A-F8", _a(8), "scattered", {}), ("A-F2-contended", _a(2), "contended", {}),
                   ("A-F4-contended", _a(4), "contended", {}), ("B", D.CONFIG_B, "scattered", {}),
                   ("one-level", D.CONFIG_ONE_LEVEL, "scattered", {}), ("32-levels", D.CONFIG_32_LEVELS, "scattered", {}),
                   ("17-levels", D.CONFIG_17_LEVELS, "coarse", dict(p_max=1, dy_den=2))]


@pytest.mark.parametrize("name,cfg,lattice,kw", CONDITION_CASES, ids=[c[0] for c in CONDITION_CASES])
def test_exact_data_keeps_every_float32_operation_exact(name, cfg, lattice, kw):
    """At the largest N the matrix runs the config with (16 385; 4099 for the deep configs), in both orders (the order changes
    no sum, only the draw): the oracle's results are float32 values, and the sums of magnitudes (plus a prefill of 4 for the
    ADDS contract) stay below 2^24 units."""
    N = 16385 if cfg["n_levels"] <= 5 else 4099
    for order in ORDERS:
        x, P, dy = D.exact_case(cfg, N, lattice, order, seed=3, **kw)
        assert float(x.min()) < 0 and float(x.max()) > 1              # cells that wrap as uint32, and cells past the grid
        cond = D.conditions(x, P, dy, cfg, lattice, kw.get("dy_den", 8), prefill=4.0)
        print(f"{name} {order}: forward 2^{_log2(cond['forward_units']):.1f}, entry sum 2^{_log2(cond['entry_units']):.1f}, "
              f"dL/dx sum 2^{_log2(cond['dx_units']):.1f} units")
        D.assert_exact(cond)
        assert np.count_nonzero(cond["gP"]) > 0 and np.count_nonzero(cond["gx"]) > 0
    if lattice == "contended":                                        # thousands of adds per entry
        lay = D.layout(cfg)
        idx, w, _ = O._corners(x, lay, 0)
        assert np.bincount(idx[w > 0]).max() >= 2000


def test_contended_lattice_is_a_handful_of_points():
    x = D.lattice_points("contended", 16385, "random", 0)
    assert len(np.unique(x, axis=0)) == D.CONTENDED_POINTS
    xs = D.lattice_points("contended", 16385, "lexsorted", 0)
    assert np.array_equal(np.unique(x, axis=0), np.unique(xs, axis=0))
    assert len(np.unique(D.lattice_points("scattered", 16385, "random", 0), axis=0)) > 3000


def _header_lds_bytes():
    text = open(os.path.join(ROOT, "tssplat_amd", "csrc", "grid.h")).read()
    m = re.search(r"constexpr\s+int\s+kGridLdsBytes\s*=\s*(\d+)\s*\*\s*(\d+)\s*;", text)
    assert m, "csrc/grid.h no longer states kGridLdsBytes as a product of two integers"
    return int(m.group(1)) * int(m.group(2))


def test_lds_global_split_sits_where_the_matrix_expects_it():
    """The library's own layout (tsamd_grid_layout) under the rule of csrc/grid_capi.cpp with the header's kGridLdsBytes: a
    change of the limit, or of a level's size, moves a split and fails here, because the matrix below would then no longer put a
    level at exactly 64 KB and exactly 128 KB, nor a hashed level on the LDS path."""
    from tssplat_amd import encoding
    lds_bytes = _header_lds_bytes()
    assert lds_bytes == D.LDS_BYTES == 128 * 1024

    def split(cfg):
        n = encoding.parse_grid_config(3, cfg)
        lay_c, lay = encoding.grid_layout(n), D.layout(cfg)
        assert np.array_equal(lay_c["offset"], lay["offset"]) and np.array_equal(lay_c["res"], lay["res"])
        assert np.array_equal(lay_c["is_hash"], lay["is_hash"]) and np.array_equal(lay_c["scale"], lay["scale"])
        assert np.array_equal(lay["scale"], np.round(lay["scale"]))                          # integer scales
        return D.lds_levels(lay, lds_bytes), (lay["entries"] * lay["F"] * 4).tolist(), lay["is_hash"].tolist()
    for F, want in LDS_SPLIT_A.items():
        got, table_bytes, hashed = split(_a(F))
        assert got == want, (F, got, table_bytes)
        assert hashed == [False, False, False, True, True]
    assert D.layout(_a(2))["entries"].tolist() == [64, 512, 4096, 16384, 16384]
    assert split(_a(1))[1][3] == 64 * 1024 and split(_a(2))[1][3] == 128 * 1024            # a hashed level, in LDS, at either edge
    assert split(_a(4))[1][2] == 64 * 1024 and split(_a(4))[1][3] > lds_bytes
    assert split(_a(8))[1][2] == 128 * 1024
    got, table_bytes, hashed = split(D.CONFIG_B)
    assert got == LDS_SPLIT_B and not any(hashed)
    lay = D.layout(D.CONFIG_B)
    assert lay["entries"].tolist() == [128, 1000, 8000, 64000]                             # `% entries`, not a mask, from level 1 on
    assert split(D.CONFIG_SECOND_TRIP)[0] == 2 and split(D.CONFIG_17_LEVELS)[0] == 17 and split(D.CONFIG_32_LEVELS)[0] == 32


def test_deepest_exact_config_the_layout_accepts():
    """per_level_scale = 2.0 and 32 levels need base * 2^31 - 1 <= 65535: the layout refuses every base.  The deepest exact
    config with that scale is base 1 with 17 levels; 32 levels are reached with per_level_scale = 1.0 (every level alike)."""
    from tssplat_amd import _capi, encoding
    for base in (1, 2, 4, 16):
        with pytest.raises(_capi.TsamdError, match="scale out of range"):
            encoding.grid_layout(encoding.parse_grid_config(3, dict(D.CONFIG_17_LEVELS, n_levels=32, base_resolution=base)))
    with pytest.raises(_capi.TsamdError, match="scale out of range"):
        encoding.grid_layout(encoding.parse_grid_config(3, dict(D.CONFIG_17_LEVELS, n_levels=18)))
    lay = encoding.grid_layout(encoding.parse_grid_config(3, D.CONFIG_17_LEVELS))
    assert lay["scale"].tolist() == [float(2 ** l - 1) for l in range(17)]
    lay = encoding.grid_layout(encoding.parse_grid_config(3, D.CONFIG_32_LEVELS))
    assert lay["scale"].tolist() == [3.0] * 32
    with pytest.raises(_capi.TsamdError, match="n_levels"):
        encoding.grid_layout(encoding.parse_grid_config(3, dict(D.CONFIG_32_LEVELS, n_levels=33)))


def _second_trip_case():
    """(x, P, dy) of the base set, R, r: N = R * base + r.  dy in {-1, 0, 1} and the m = 1 lattice: a unit of 2^-3."""
    x, P, dy = D.exact_case(D.CONFIG_SECOND_TRIP, SECOND_TRIP_BASE, "coarse", "random", seed=5, dy_den=1)
    return x, P, dy, SECOND_TRIP_N // SECOND_TRIP_BASE, SECOND_TRIP_N % SECOND_TRIP_BASE


def _second_trip_expected():
    x, P, dy, R, r = _second_trip_case()
    lay = D.layout(D.CONFIG_SECOND_TRIP)
    full, _ = O.encode_backward(x, P, dy, lay)
    head, _ = O.encode_backward(x[:r], P, dy[:r], lay)
    abs_full, _ = O.encode_backward(x, P, np.abs(dy), lay)
    abs_head, _ = O.encode_backward(x[:r], P, np.abs(dy[:r]), lay)
    return R * full + head, float((R * abs_full + abs_head).max()) * 2.0 ** 3


def test_tiling_identity_the_second_trip_case_rests_on():
    """dL/dparams of R copies of a base set plus its first r points is R gP(base) + gP(base[:r]), every term exact in float64:
    checked on the oracle itself with R = 3, and the 2^24-unit condition at the full N."""
    x, P, dy, R, r = _second_trip_case()
    assert R * SECOND_TRIP_BASE + r == SECOND_TRIP_N and 0 < r < SECOND_TRIP_BASE and R > 1000
    lay = D.layout(D.CONFIG_SECOND_TRIP)
    full, _ = O.encode_backward(x, P, dy, lay)
    head, _ = O.encode_backward(x[:r], P, dy[:r], lay)
    tiled, _ = O.encode_backward(np.concatenate([x] * 3 + [x[:r]]), P, np.concatenate([dy] * 3 + [dy[:r]]), lay)
    assert np.array_equal(tiled, 3 * full + head)
    want, units = _second_trip_expected()
    print(f"second trip: N = {SECOND_TRIP_N}, largest entry sum 2^{_log2(units):.1f} units of 2^-3")
    assert units < 2 ** 24 and np.array_equal(want.astype(np.float32).astype(np.float64), want) and np.count_nonzero(want) > 20


# ------------------------------------------------------------------------------------------------------------------ GPU tier
def _enc(cfg, P, param_grad="atomic"):
    from tssplat_amd import encoding
    enc = encoding.GridEncoding(3, cfg, param_grad=param_grad).cuda()
    with torch.no_grad():
        enc.params.copy_(torch.from_numpy(P))
    return enc


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def _same(got, want64, what):
    got, want = got.detach().cpu().numpy(), _f32(want64).reshape(tuple(got.shape))
    assert np.array_equal(got, want), (what, int((got != want).sum()), float(np.abs(got.astype(np.float64) - want).max()))


def _assert_all_routes_exact(cfg, x, P, dy, lattice, dy_den=8):
    """Forward, dL/dparams by the three routes and dL/dx of the HIP encoding equal the oracle rounded to float32, bit for bit."""
    cond = D.conditions(x, P, dy, cfg, lattice, dy_den)
    D.assert_exact(cond)
    xd, dyd = torch.from_numpy(x).cuda(), torch.from_numpy(dy).cuda()
    for mode in ("atomic", "sorted"):
        enc = _enc(cfg, P, mode)
        xg = xd.clone().requires_grad_(True)
        out = enc(xg)
        out.backward(dyd)
        _same(out, cond["y"], f"forward ({mode})")
        _same(enc.params.grad, cond["gP"], f"dL/dparams ({mode})")
        _same(xg.grad, cond["gx"], f"dL/dx ({mode})")
    enc = _enc(cfg, P)
    out = enc(enc.plan_points(xd))
    out.backward(dyd)
    _same(out, cond["y"], "forward (planned)")
    _same(enc.params.grad, cond["gP"], "dL/dparams (planned)")


@pytest.mark.gpu
@pytest.mark.parametrize("N", EDGES)
@pytest.mark.parametrize("lattice", ["scattered", "contended"])
@pytest.mark.parametrize("F", [2, 4])
def test_config_a_at_every_launch_edge(F, lattice, N):
    """F = 2: all five levels through the LDS kernel, the two hashed ones at exactly 128 KB.  F = 4: three levels in LDS, the
    hashed two through the global atomic kernel.  Every route, both point orders."""
    assert D.lds_levels(D.layout(_a(F))) == LDS_SPLIT_A[F]
    for order in ORDERS:
        _assert_all_routes_exact(_a(F), *D.exact_case(_a(F), N, lattice, order, seed=N), lattice)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [65, 1025, 16385])
@pytest.mark.parametrize("F", [1, 8])
def test_config_a_other_feature_widths(F, N):
    """F = 1: a hashed level of exactly 64 KB in LDS, launched without the dynamic-LDS attribute.  F = 8: level 2 at exactly
    128 KB, float4 pairs per entry."""
    assert D.lds_levels(D.layout(_a(F))) == LDS_SPLIT_A[F]
    for lattice in ("scattered", "contended"):
        for order in ORDERS:
            _assert_all_routes_exact(_a(F), *D.exact_case(_a(F), N, lattice, order, seed=N + F), lattice)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [65, 257, 4099, 16385])
def test_dense_grid_through_every_route(N):
    """DenseGrid, entries 128, 1000, 8000, 64000: the true `% entries` of corner_index, three levels in LDS and one global."""
    for order in ORDERS:
        _assert_all_routes_exact(D.CONFIG_B, *D.exact_case(D.CONFIG_B, N, "scattered", order, seed=N), "scattered")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one-level", "17-levels", "32-levels"])
def test_level_counts(name):
    """One level; the deepest exact config with per_level_scale = 2.0 (17 levels, scale up to 65535: coarser data keep dL/dx
    below 2^24 units); 32 levels, the whole level table of the kernels, with per_level_scale = 1.0."""
    _, cfg, lattice, kw = next(c for c in CONDITION_CASES if c[0] == name)
    for order in ORDERS:
        for N in (65, 4099):
            _assert_all_routes_exact(cfg, *D.exact_case(cfg, N, lattice, order, seed=N, **kw), lattice, kw.get("dy_den", 8))


@pytest.mark.gpu
def test_lds_kernel_past_its_workgroup_cap():
    """N = 256 * 16384 + 65: the LDS kernel runs its 256 workgroups (the cap) and its grid-stride loop goes one trip past the 16
    that ceil(N / 16384) workgroups make below the cap; the last wave is partly filled.  x is R copies of a base set plus its
    first r points, tiled on the device; the expected dL/dparams is R gP(base) + gP(base[:r]) from two small oracle calls."""
    from tssplat_amd import _capi, encoding
    lib = _capi.load()
    x, P, dy, R, r = _second_trip_case()
    want, units = _second_trip_expected()
    assert units < 2 ** 24
    cfg = encoding.parse_grid_config(3, D.CONFIG_SECOND_TRIP)
    xb, dyb, Pd = torch.from_numpy(x).cuda(), torch.from_numpy(dy).cuda(), torch.from_numpy(P).cuda()
    xd = torch.cat([xb.repeat(R, 1), xb[:r]]).contiguous()
    dyd = torch.cat([dyb.repeat(R, 1), dyb[:r]]).contiguous()
    assert xd.shape == (SECOND_TRIP_N, 3) and dyd.shape == (SECOND_TRIP_N, 2)
    grad_p = torch.zeros_like(Pd)
    torch.cuda.synchronize()
    _capi.check(lib.tsamd_grid_encode_backward(xd.data_ptr(), SECOND_TRIP_N, Pd.data_ptr(), *encoding._args(cfg), dyd.data_ptr(),
                                               grad_p.data_ptr(), None, None))
    torch.cuda.synchronize()
    _same(grad_p, want, "dL/dparams (atomic, 4 M points)")


# ------------------------------------------------------------------------------------------------ contracts through the C ABI
CONTRACT_F, CONTRACT_N = 4, 4099         # F = 4: the LDS and the global atomic kernel both run


@pytest.fixture(scope="module")
def contract():
    """Config A at F = 4 on the device, with the oracle's answers (computed once, left unchanged)."""
    from tssplat_amd import encoding
    cfg = _a(CONTRACT_F)
    x, P, dy = D.exact_case(cfg, CONTRACT_N, "scattered", "random", seed=77)
    cond = D.conditions(x, P, dy, cfg, "scattered", prefill=4.0)
    D.assert_exact(cond)
    n = encoding.parse_grid_config(3, cfg)
    dev = {k: torch.from_numpy(v).cuda() for k, v in (("x", x), ("P", P), ("dy", dy))}
    return {"cfg": cfg, "n": n, "x": x, "P": P, "dy": dy, "cond": cond, "dev": dev, "args": encoding._args(n)}


def _abi_backward(route, c, grad_p, grad_x):
    """One backward entry point of the C ABI on the contract case; grad_p / grad_x: device tensors or None (NULL)."""
    from tssplat_amd import _capi, encoding
    lib = _capi.load()
    d, n, N = c["dev"], c["n"], CONTRACT_N
    ptr = lambda t: None if t is None else t.data_ptr()
    torch.cuda.synchronize()
    if route == "atomic":
        rc = lib.tsamd_grid_encode_backward(d["x"].data_ptr(), N, d["P"].data_ptr(), *c["args"], d["dy"].data_ptr(), ptr(grad_p), ptr(grad_x), None)
    elif route == "sorted":
        ws = torch.empty(encoding.sorted_workspace_bytes(n, N) if grad_p is not None else 0, dtype=torch.uint8, device="cuda")
        rc = lib.tsamd_grid_encode_backward_sorted(d["x"].data_ptr(), N, d["P"].data_ptr(), *c["args"], d["dy"].data_ptr(), ptr(grad_p),
                                                   ptr(grad_x), ws.data_ptr() if ws.numel() else None, ws.numel(), None)
    else:
        plan = encoding.GridPointPlan(d["x"], n)
        ws = torch.empty(encoding.planned_workspace_bytes(n, N), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rc = lib.tsamd_grid_encode_backward_planned(d["x"].data_ptr(), N, *c["args"], d["dy"].data_ptr(), ptr(grad_p), plan.buffer.data_ptr(),
                                                    plan.buffer.numel(), ws.data_ptr(), ws.numel(), None)
    _capi.check(rc)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["atomic", "sorted", "planned"])
def test_backward_adds_into_grad_params(contract, route):
    """csrc/grid.h: every backward ADDS.  grad_params starts as small integers (autograd only ever hands in zeros); afterwards it
    is prefill + oracle, bit for bit -- twice in a row, so the second call adds onto the first one's result."""
    rng = np.random.default_rng(9)
    prefill = rng.integers(-4, 5, contract["P"].shape[0]).astype(np.float32)
    grad_p = torch.from_numpy(prefill).cuda()
    _abi_backward(route, contract, grad_p, None)
    _same(grad_p, prefill.astype(np.float64) + contract["cond"]["gP"], f"prefill + dL/dparams ({route})")
    assert contract["cond"]["entry_units"] * 2 < 2 ** 24
    _abi_backward(route, contract, grad_p, None)
    _same(grad_p, prefill.astype(np.float64) + 2 * contract["cond"]["gP"], f"prefill + 2 dL/dparams ({route})")


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["atomic", "sorted"])
def test_grad_x_null_and_grad_params_null_are_launch_paths_of_their_own(contract, route):
    """grad_x == NULL: dL/dparams alone, and a canary where dL/dx would go stays untouched.  grad_params == NULL: dL/dx alone
    (the sorted entry point then needs no workspace).  Both at once: nothing to do."""
    N = CONTRACT_N
    grad_p = torch.zeros_like(contract["dev"]["P"])
    _abi_backward(route, contract, grad_p, None)
    _same(grad_p, contract["cond"]["gP"], f"dL/dparams alone ({route})")
    grad_x = torch.full((N + 2, 3), 7.0, dtype=torch.float32, device="cuda")               # a canary row on either side
    _abi_backward(route, contract, None, grad_x[1:N + 1])
    _same(grad_x[1:N + 1], contract["cond"]["gx"], f"dL/dx alone ({route})")
    assert bool((grad_x[0] == 7.0).all()) and bool((grad_x[N + 1] == 7.0).all())
    _abi_backward(route, contract, None, None)
    both_p, both_x = torch.zeros_like(grad_p), torch.empty(N, 3, dtype=torch.float32, device="cuda")
    _abi_backward(route, contract, both_p, both_x)
    _same(both_p, contract["cond"]["gP"], f"dL/dparams with dL/dx ({route})")
    _same(both_x, contract["cond"]["gx"], f"dL/dx with dL/dparams ({route})")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["atomic", "sorted"])
def test_x_without_gradient_and_frozen_params_through_autograd(contract, mode, monkeypatch):
    """x carries no gradient: dL/dparams is the oracle's.  Params frozen, x requires a gradient: the sorted mode takes the atomic
    entry point (it has nothing to sort), dL/dx keeps its bits and params.grad stays None."""
    from tssplat_amd import encoding
    d, cond = contract["dev"], contract["cond"]
    enc = _enc(contract["cfg"], contract["P"], mode)
    out = enc(d["x"])
    out.backward(d["dy"])
    _same(out, cond["y"], f"forward ({mode})")
    _same(enc.params.grad, cond["gP"], f"dL/dparams, x without gradient ({mode})")
    assert d["x"].grad is None

    calls = {"atomic": 0, "sorted": 0}
    atomic_entry, sorted_entry = encoding._lib.tsamd_grid_encode_backward, encoding._lib.tsamd_grid_encode_backward_sorted

    def count(name, entry):
        def call(*args):
            calls[name] += 1
            return entry(*args)
        return call
    monkeypatch.setattr(encoding._lib, "tsamd_grid_encode_backward", count("atomic", atomic_entry))
    monkeypatch.setattr(encoding._lib, "tsamd_grid_encode_backward_sorted", count("sorted", sorted_entry))
    frozen = _enc(contract["cfg"], contract["P"], mode)
    frozen.params.requires_grad_(False)
    xg = d["x"].clone().requires_grad_(True)
    frozen(xg).backward(d["dy"])
    assert calls == {"atomic": 1, "sorted": 0}
    assert frozen.params.grad is None
    _same(xg.grad, cond["gx"], f"dL/dx, frozen params ({mode})")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["atomic", "sorted"])
def test_non_contiguous_x_and_upstream_gradient(contract, mode):
    """x as a column slice of a wider tensor, dy as the transpose of a [C, N] tensor and as an expanded row: the bits of the
    contiguous run, which are the oracle's."""
    cond, cfg, N = contract["cond"], contract["cfg"], CONTRACT_N
    wide = torch.full((N, 5), 0.3125, dtype=torch.float32, device="cuda")
    wide[:, 1:4] = contract["dev"]["x"]
    wide.requires_grad_(True)
    x = wide[:, 1:4]
    dy_t = contract["dev"]["dy"].t().contiguous().t()
    assert not x.is_contiguous() and not dy_t.is_contiguous() and torch.equal(dy_t, contract["dev"]["dy"])
    enc = _enc(cfg, contract["P"], mode)
    out = enc(x)
    out.backward(dy_t)
    _same(out, cond["y"], f"forward, sliced x ({mode})")
    _same(enc.params.grad, cond["gP"], f"dL/dparams, sliced x and transposed dy ({mode})")
    _same(wide.grad[:, 1:4], cond["gx"], f"dL/dx, sliced x and transposed dy ({mode})")
    assert not bool(wide.grad[:, 0].any()) and not bool(wide.grad[:, 4].any())
    # an expanded row: every point gets the same upstream gradient
    row = contract["dy"][:1]
    dy_rows = np.ascontiguousarray(np.broadcast_to(row, contract["dy"].shape))
    want = D.conditions(contract["x"], contract["P"], dy_rows, cfg, "scattered")
    D.assert_exact(want)
    expanded = torch.from_numpy(row).cuda().expand(N, -1)
    assert not expanded.is_contiguous()
    enc = _enc(cfg, contract["P"], mode)
    xg = contract["dev"]["x"].clone().requires_grad_(True)
    enc(xg).backward(expanded)
    _same(enc.params.grad, want["gP"], f"dL/dparams, expanded dy ({mode})")
    _same(xg.grad, want["gx"], f"dL/dx, expanded dy ({mode})")


# ------------------------------------------------------------------------------------- random data: derived rounding bounds
U = 2.0 ** -24                       # the unit roundoff of float32


def _gamma(k):
    return k * U / (1 - k * U)       # (1 + u)^k - 1 <= gamma_k: k roundings in a row, second-order terms included


def _random_case(F, seed):
    cfg = _a(F)
    lay = D.layout(cfg)
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.02, 1.02, (4099, 3)).astype(np.float32)
    P = rng.uniform(-1, 1, lay["n_params"]).astype(np.float32)
    dy = rng.normal(size=(4099, lay["L"] * F)).astype(np.float32)
    return cfg, lay, x, P, dy


@pytest.mark.gpu
@pytest.mark.parametrize("F", [1, 2, 4, 8])
def test_random_forward_within_the_derived_bound(F):
    """|y - ref| <= gamma(k_f) sum_c w_c |v_c| for EVERY element, k_f = 13, counted on grid_encode_kernel:

    * pos, floor and frac are the oracle's own float32 values (frac = pos - floor(pos) is one float32 subtraction in both), so
      the cell and the frac are identical: 0 roundings, no point can change its cell;
    * a weight factor is f or 1 - f: at most 1 rounding per axis, 3 per corner weight;
    * wx * wy * wz: 2 roundings.  The float32 weight is w_c (1 + d)^5;
    * acc = fmaf(w_c, v_c, acc), 8 in a row from acc = 0: the term of corner c is rounded by its own fma and by every later
      one, at most 8 times (the corner-0 term).
    3 + 2 + 8 = 13 factors (1 + d) on every term w_c v_c.  The oracle's float64 error is 2^-29 of that."""
    k_f = 3 + 2 + 8
    cfg, lay, x, P, dy = _random_case(F, 40 + F)
    ref = O.encode(x, P, lay)
    mag = O.encode(x, np.abs(P), lay)
    out = _enc(cfg, P)(torch.from_numpy(x).cuda()).detach().cpu().double().numpy()
    err, bound = np.abs(out - ref), _gamma(k_f) * mag
    print(f"forward F = {F}: k_f = {k_f}, max err / bound = {(err / bound).max():.3f}, max err {err.max():.3e}")
    assert np.all(mag > 0) and np.all(err <= bound), (float((err / bound).max()), int((err > bound).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("F", [1, 2, 4, 8])
def test_random_input_gradient_within_the_derived_bound(F):
    """|g - ref| <= gamma(k_x) sum_l scale_l sum_c sum_f |v_cf g_f| |d w_c / d pos_d| for EVERY point and axis,
    k_x = F + 12 + L, counted on grid_backward_x_kernel (axis 0; the others alike):

    * cell and frac identical to the oracle's, as in the forward: 0;
    * s = fmaf(v_f, g_f, s), F in a row from 0: a term v_f g_f is rounded at most F times;
    * wy and wz are f or 1 - f: 1 rounding each, 2;
    * (+-s) * wy * wz: 2 roundings (1 if the compiler fuses the second product with the add; 2 covers both);
    * gl += ..., 8 in a row from 0: a corner's term is rounded by its own add and by every later one, at most 8 times;
    * gx = fmaf(gl, scale_l, gx), L in a row from 0: level l's term is rounded by its own fma and by every later one, at
      most L times (level 0's).
    F + 2 + 2 + 8 + L factors (1 + d) on every term v_cf g_f dw_c scale_l."""
    cfg, lay, x, P, dy = _random_case(F, 50 + F)
    k_x = F + 2 + 2 + 8 + lay["L"]
    _, ref = O.encode_backward(x, P, dy, lay)
    mag = D.dx_abs_sum(x, P, dy, lay)
    enc = _enc(cfg, P)
    xg = torch.from_numpy(x).cuda().requires_grad_(True)
    enc(xg).backward(torch.from_numpy(dy).cuda())
    err, bound = np.abs(xg.grad.cpu().double().numpy() - ref), _gamma(k_x) * mag
    print(f"dL/dx F = {F}: k_x = {k_x}, max err / bound = {(err / bound).max():.3f}, max err {err.max():.3e}")
    assert np.all(mag > 0) and np.all(err <= bound), (float((err / bound).max()), int((err > bound).sum()))


# ------------------------------------------------------------------------------------------- inputs outside the defined domain
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["atomic", "sorted"])
def test_rows_outside_the_domain_leave_the_other_rows_alone(mode):
    """+-inf, NaN and |scale x + 0.5| >= 2^31 among exact rows (N = 65): those rows' values are unspecified (the oracle wraps, the
    device conversion saturates; every index is still reduced modulo the entry count, so all accesses stay in bounds).  The
    forward and dL/dx of the in-domain rows are bitwise what a run without the wild rows gives, and the oracle's.  dL/dparams
    is computed (the wild rows go through both backward kernels) but not compared."""
    cfg = _a(4)
    x, P, dy = D.exact_case(cfg, 65, "scattered", "random", seed=65)
    wild = {3: [np.inf, 0.5, 0.5], 17: [0.25, -np.inf, 0.125], 31: [np.nan, np.nan, np.nan], 40: [0.5, 0.5, 4e9],
            63: [-3e38, 3e38, 0.5], 64: [2.0 ** 31, 0.25, np.nan]}
    xw = x.copy()
    for row, v in wild.items():
        xw[row] = v
    lay = D.layout(cfg)
    assert all(np.isnan(xw[r]).any() or (np.abs(lay["scale"][-1] * xw[r].astype(np.float64) + 0.5) >= 2.0 ** 31).any() for r in wild)
    keep = np.array([i for i in range(65) if i not in wild])
    cond = D.conditions(x, P, dy, cfg, "scattered")
    D.assert_exact(cond)
    got = {}
    for name, pts in (("tame", x), ("wild", xw)):
        enc = _enc(cfg, P, mode)
        xg = torch.from_numpy(pts).cuda().requires_grad_(True)
        out = enc(xg)
        out.backward(torch.from_numpy(dy).cuda())
        torch.cuda.synchronize()
        got[name] = (out.detach()[keep], xg.grad[keep])
        assert enc.params.grad.shape == (lay["n_params"],)
    assert torch.equal(got["wild"][0], got["tame"][0]) and torch.equal(got["wild"][1], got["tame"][1])
    _same(got["wild"][0], cond["y"][keep], f"forward of the in-domain rows ({mode})")
    _same(got["wild"][1], cond["gx"][keep], f"dL/dx of the in-domain rows ({mode})")
