"""``dr.texture`` (csrc/texture_kernels.hip) against tests/texture_oracle.py: bit for bit on exact data (small-integer textures,
dyadic weights, dy = k / 128: every product and every sum is exact in fp32, whatever the order of the atomics), within derived
rounding bounds on random data; the autograd surface; the kernels' descriptors."""
import os
import sys

import numpy as np
import pytest

import texture_oracle as TO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTERS, BOUNDARIES = ("nearest", "linear"), ("wrap", "clamp", "zero")
TEX_H, TEX_W = 5, 8                                                # a non-square texture


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="needs the ROCm LLVM tools")
def test_texture_and_atlas_kernels_use_no_lds_no_scratch_and_do_not_spill():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_metadata
    from tssplat_amd import _capi
    _capi.load()
    meta = kernel_metadata.kernel_metadata(_capi.lib_path())
    mine = {k: v for k, v in meta.items() if "texture_" in k or "atlas_bake" in k}
    for kernel in ("atlas_bake_kernel", "texture_nearest_kernel", "texture_nearest_backward_kernel", "texture_linear_kernel",
                   "texture_linear_backward_kernel"):
        assert sum(kernel + "E" in k for k in mine) == 1, (kernel, sorted(mine))
    for name, rec in mine.items():
        assert rec["group_segment_fixed_size"] == 0, (name, rec)
        assert rec["vgpr_spill_count"] == 0 and rec["private_segment_fixed_size"] == 0, (name, rec)
        assert rec["vgpr_count"] <= 64, (name, rec)                # eight waves per SIMD


def test_texture_translation_unit_is_built_without_fp_contraction():
    """x = u W - 0.5 is a rounded product and then a difference, as the oracle states it."""
    from tssplat_amd import _build
    assert "texture_kernels.hip" in _build.SOURCES and "texture_capi.cpp" in _build.SOURCES and "texture.h" in _build.HEADERS
    assert _build.SOURCE_FLAGS.get("texture_kernels.hip") == ["-ffp-contract=off"]


# ---------------------------------------------------------------------------------------------------------------- exact data

def _exact_uv(rng, B, h, w):
    """uv with u W - 0.5 and v H - 0.5 exact multiples of 1/4 IN REAL ARITHMETIC (so also in fp32, fused or not): W = 8 makes
    u = (x + 0.5) / 8 a dyadic number for every multiple x of 1/4; H = 5 does so for v = k / 4 (y = 1.25 k - 0.5: -0.5, 0.75, 2,
    3.25, 4.5, ...).  Ranges reach below 0 and above 1; texel centres (integer x, y) and texel edges (x, y = m + 0.5) are among
    the values, and the first pixels are pinned to them."""
    x = rng.integers(-4 * (TEX_W + 3), 4 * (2 * TEX_W + 3), size=(B, h, w)) / 4.0
    k = rng.integers(-7, 12, size=(B, h, w))
    x.reshape(-1)[:6] = [3.0, 2.5, -0.5, TEX_W - 0.5, -3.0, TEX_W + 2.5]       # centre, edge, the texture's borders, outside
    k.reshape(-1)[:6] = [2, 0, 4, 2, -2, 6]                                     # y = 2 (centre), -0.5, 4.5 (borders), ...
    uv = np.stack([(x + 0.5) / TEX_W, k / 4.0], -1).astype(np.float32)
    assert np.array_equal(uv[..., 0].astype(np.float64) * TEX_W - 0.5, x)
    assert np.array_equal((uv[..., 1].astype(np.float64) * TEX_H - 0.5) * 4, 5.0 * k - 2)
    return uv


def _one_texel_uv(B, h, w, linear):
    """All pixels on one texel: the contended add.  Linear: x = 3.25, y = 2 (weights 3/4 and 1/4 on two texels)."""
    uv = np.empty((B, h, w, 2), np.float32)
    uv[..., 0] = (3.25 + 0.5) / TEX_W if linear else 3.5 / TEX_W
    uv[..., 1] = 0.5
    return uv


def _run(tex, uv, dy, filter_mode, boundary, tex_grad=True, uv_grad=True):
    import torch
    from tssplat_amd import dr
    t = torch.from_numpy(tex).cuda().requires_grad_(tex_grad)
    p = torch.from_numpy(uv).cuda().requires_grad_(uv_grad)
    out = dr.texture(t, p, filter_mode=filter_mode, boundary_mode=boundary)
    if tex_grad or uv_grad:
        out.backward(torch.from_numpy(dy).cuda())
    return out.detach().cpu().numpy(), None if t.grad is None else t.grad.cpu().numpy(), None if p.grad is None else p.grad.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("filter_mode", FILTERS)
def test_exact_data_bit_for_bit(filter_mode, boundary):
    """tex batch 1 and B, C in {1, 3, 4}, outputs of 1 x 7 x 9 (less than a wave) and 3 x 33 x 65 (more than one workgroup, a
    ragged tail), scattered pixels and all pixels on one texel.  Sums stay far below 2^24 units of 2^-11 (the smallest product
    of a weight k / 16 and dy = k / 128): 6435 pixels x 1/2 = 3218 < 2^13."""
    rng = np.random.default_rng(5)
    linear = filter_mode == "linear"
    for (B, h, w) in ((1, 7, 9), (3, 33, 65)):
        for Cn in (1, 3, 4):
            for TB in sorted({1, B}):
                for contended in (False, True):
                    tex = rng.integers(-4, 5, size=(TB, TEX_H, TEX_W, Cn)).astype(np.float32)
                    uv = _one_texel_uv(B, h, w, linear) if contended else _exact_uv(rng, B, h, w)
                    dy = (rng.integers(-64, 65, size=(B, h, w, Cn)) / 128.0).astype(np.float32)
                    out, g_tex, g_uv = _run(tex, uv, dy, filter_mode, boundary)
                    want = TO.forward(tex, uv, filter_mode, boundary)
                    want_tex, want_uv, _, n_adds = TO.backward(tex, uv, dy, filter_mode, boundary)
                    where = (filter_mode, boundary, B, h, w, Cn, TB, contended)
                    assert out.shape == (B, h, w, Cn) and np.array_equal(out, want.astype(np.float32)), where
                    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)          # (the data is exact)
                    assert g_tex.shape == tex.shape and np.array_equal(g_tex, want_tex.astype(np.float32)), where
                    if linear:
                        assert g_uv.shape == uv.shape and np.array_equal(g_uv, want_uv.astype(np.float32)), where
                    else:
                        assert g_uv is None, where
                    if contended:
                        assert n_adds.max() == (B * h * w if TB == 1 else h * w), where       # adds into one texture element


@pytest.mark.gpu
def test_boundary_modes_on_a_hand_made_case():
    """One row of four texels 10, 20, 30, 40 sampled off both ends: what wrap / clamp / zero mean, spelled out."""
    tex = np.array([10, 20, 30, 40], np.float32).reshape(1, 1, 4, 1)
    u = np.array([-0.125, 0.125, 0.875, 1.125, -1.0], np.float32)              # x = -1, 0, 3, 4, -4.5
    uv = np.stack([u, np.full_like(u, 0.5)], -1).reshape(1, 1, 5, 2)
    dy = np.ones((1, 1, 5, 1), np.float32)
    expect = {("linear", "wrap"): [40, 10, 40, 10, 25], ("linear", "clamp"): [10, 10, 40, 40, 10], ("linear", "zero"): [0, 10, 40, 0, 0],
              ("nearest", "wrap"): [40, 10, 40, 10, 10], ("nearest", "clamp"): [10, 10, 40, 40, 10], ("nearest", "zero"): [0, 10, 40, 0, 0]}
    for (filter_mode, boundary), want in expect.items():
        out, g_tex, g_uv = _run(tex, uv, dy, filter_mode, boundary)
        assert out.reshape(-1).tolist() == want, (filter_mode, boundary)
        assert np.array_equal(out, TO.forward(tex, uv, filter_mode, boundary).astype(np.float32))
    # clamp, linear, off the end: both taps are the same texel, so the uv gradient is 0; wrap sees 40 -> 10 across the seam
    _, _, g_uv = _run(tex, uv, dy, "linear", "clamp")
    assert g_uv[0, 0, :, 0].tolist() == [0.0, 4 * 10.0, 4 * 0.0, 0.0, 0.0]
    _, _, g_uv = _run(tex, uv, dy, "linear", "wrap")
    assert g_uv[0, 0, :, 0].tolist() == [4 * -30.0, 4 * 10.0, 4 * -30.0, 4 * 10.0, 4 * -30.0]


# ---------------------------------------------------------------------------------------------------------------- autograd surface

@pytest.mark.gpu
def test_autograd_combinations_and_what_is_refused():
    import torch
    from tssplat_amd import dr
    rng = np.random.default_rng(9)
    tex = rng.integers(-4, 5, size=(1, TEX_H, TEX_W, 3)).astype(np.float32)
    uv = _exact_uv(rng, 2, 7, 9)
    dy = (rng.integers(-64, 65, size=(2, 7, 9, 3)) / 128.0).astype(np.float32)
    for filter_mode in FILTERS:
        want_tex, want_uv, _, _ = TO.backward(tex, uv, dy, filter_mode, "wrap")
        for tex_grad in (False, True):
            for uv_grad in (False, True):
                out, g_tex, g_uv = _run(tex, uv, dy, filter_mode, "wrap", tex_grad, uv_grad)
                assert np.array_equal(out, TO.forward(tex, uv, filter_mode, "wrap").astype(np.float32))
                assert (g_tex is not None) == tex_grad and (g_uv is not None) == (uv_grad and filter_mode == "linear")
                if g_tex is not None:
                    assert np.array_equal(g_tex, want_tex.astype(np.float32))
                if g_uv is not None:
                    assert np.array_equal(g_uv, want_uv.astype(np.float32))
    t, p = torch.from_numpy(tex).cuda(), torch.from_numpy(uv).cuda()
    assert not dr.texture(t, p).requires_grad
    assert torch.equal(dr.texture(t, p), dr.texture(t, p, filter_mode="linear", boundary_mode="wrap"))     # 'auto' = 'linear'
    assert "texture" in dr.__all__
    for kwargs in ({"uv_da": p}, {"mip_level_bias": p[..., :1]}, {"mip": [t]}, {"max_mip_level": 2}, {"filter_mode": "linear-mipmap-nearest"},
                   {"filter_mode": "linear-mipmap-linear"}, {"boundary_mode": "cube"}):
        with pytest.raises(NotImplementedError):
            dr.texture(t, p, **kwargs)
    with pytest.raises(ValueError):
        dr.texture(t, p, filter_mode="cubic")
    with pytest.raises(RuntimeError):
        dr.texture(t.cpu(), p)
    with pytest.raises(RuntimeError):
        dr.texture(t.expand(3, -1, -1, -1), p)                     # tex batch neither 1 nor B


# ---------------------------------------------------------------------------------------------------------------- random data

def _adjacent_step(tex, boundary):
    """D: the largest difference between adjacent texels, neighbours across the border as the boundary mode defines them."""
    mode = {"wrap": dict(mode="wrap"), "clamp": dict(mode="edge"), "zero": dict(mode="constant", constant_values=0.0)}[boundary]
    t = np.pad(tex.astype(np.float64), ((0, 0), (1, 1), (1, 1), (0, 0)), **mode)
    return max(np.abs(np.diff(t, axis=1)).max(), np.abs(np.diff(t, axis=2)).max())


def _random_case(rng, boundary, TB, Cn):
    """tex [TB, 13, 11, Cn] normal; uv [2, 37, 41, 2] with u W in [-0.95 W, W] -- so |u W| and |x| stay <= W, which is what the
    2^-23 (W + H) of the bounds assumes -- and its fractional part kept in [0.05, 0.45] or [0.55, 0.95]: nearest is discontinuous
    where u W is an integer, the uv gradient where u W - 0.5 is, and the kernel's fp32 coordinate may fall on the other side."""
    H, W, B, h, w = 13, 11, 2, 37, 41
    tex = rng.normal(size=(TB, H, W, Cn)).astype(np.float32)
    cells = np.stack([rng.integers(-W + 1, W, size=(B, h, w)), rng.integers(-H + 1, H, size=(B, h, w))], -1)
    frac = rng.uniform(0.05, 0.45, size=(B, h, w, 2)) + 0.5 * rng.integers(0, 2, size=(B, h, w, 2))
    uv = ((cells + frac) / np.array([W, H])).astype(np.float32)
    dy = rng.normal(size=(B, h, w, Cn)).astype(np.float32)
    return tex, uv, dy


@pytest.mark.gpu
@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("filter_mode", FILTERS)
def test_random_data_within_rounding_bounds(filter_mode, boundary):
    rng = np.random.default_rng(21)
    e = 2.0 ** -24                                                  # one fp32 rounding, relative
    for TB, Cn in ((1, 3), (2, 4), (2, 1)):
        tex, uv, dy = _random_case(rng, boundary, TB, Cn)
        _, H, W, _ = tex.shape
        out, g_tex, g_uv = _run(tex, uv, dy, filter_mode, boundary)
        want = TO.forward(tex, uv, filter_mode, boundary)
        want_tex, want_uv, abs_adds, n_adds = TO.backward(tex, uv, dy, filter_mode, boundary)
        D, tmax = _adjacent_step(tex, boundary), float(np.abs(tex).max())
        # x = fl(fl(u W) - 0.5) is off by at most e (|u W| + |x|) <= 2 e W, y by 2 e H; the sampled value is continuous and
        # piecewise bilinear with slopes of at most D per texel: 2 e (W + H) D.  Weights, products and sums: at most 8 roundings
        # of terms bounded by max|tex|.
        bound = 2 * e * (W + H) * D + 8 * e * tmax if filter_mode == "linear" else 0.0       # (nearest copies a texel)
        err = np.abs(out - want).max()
        print(f"{filter_mode} {boundary} TB={TB} C={Cn}: forward err {err:.3e} <= {bound:.3e}")
        assert err <= bound
        # grad_tex: a contribution w g has a weight that is off by at most 2 e (W + H) (|dw/dx|, |dw/dy| <= 1) plus 3 roundings
        # (1 - f, the product of the two factors, the product with g); the fp32 accumulation of n contributions in any order
        # adds at most e n sum|w g|.  sum|g| over the contributing pixels is at most sum|w g| / min w, but the first term needs
        # no weight: it is bounded through the pixels' |g| scattered to their taps.
        g_abs = np.abs(dy.astype(np.float64))
        tb, taps, _ = TO._taps(tex.shape, uv, filter_mode, boundary)
        sum_g = np.zeros_like(want_tex)
        for ry, rx, exists, wgt in taps:
            np.add.at(sum_g, (tb, ry, rx), (exists & (wgt != 0))[..., None] * g_abs)
        bound_tex = (2 * e * (W + H) * sum_g if filter_mode == "linear" else 0.0) + e * (n_adds + 3) * abs_adds
        err_tex = np.abs(g_tex - want_tex)
        print(f"    grad_tex err {err_tex.max():.3e}, max err / bound {np.max(err_tex / np.maximum(bound_tex, 1e-300)):.3f}")
        assert (err_tex <= bound_tex).all()
        if filter_mode == "nearest":
            assert g_uv is None
            continue
        # grad_uv: du = W sum_c g_c ((t10 - t00)(1 - fy) + (t11 - t01) fy).  fy is off by at most 2 e H and multiplies the mixed
        # difference (t11 - t01) - (t10 - t00), at most 2 D; the two differences, 1 - fy, two products, their sum, the product
        # with g, the sum over C <= 4 channels and the product with W: at most 12 roundings of terms bounded by D |g|; 16 taken.
        sg = g_abs.sum(-1)
        bound_uv = np.stack([W * sg * D * (2 * e * H * 2 + 16 * e), H * sg * D * (2 * e * W * 2 + 16 * e)], -1)
        err_uv = np.abs(g_uv - want_uv)
        print(f"    grad_uv err {err_uv.max():.3e}, max err / bound {np.max(err_uv / bound_uv):.3f}")
        assert (err_uv <= bound_uv).all()
