"""The depth term without an image chain: tsamd_depth_mse / tsamd_depth_mse_backward, dr.silhouette_depth_mse and
MeshRasterizer.silhouette_depth_loss against the operator chain (rasterize -> interpolate -> norm -> masked MSELoss) and its
float64 restatement (tests/depth_oracle.py over oracle/raster_oracle.py).

CPU tier: the argument checks of the C ABI, and the oracle's own ``grad_world`` against central differences (ids frozen).  The
clip positions are NOT finite-differenced: the backward treats the clamps of (u, v) as inactive by definition, which a difference
quotient does not (it disagrees by 5e-3 .. 3e-2 where a diagonal passes through pixel centres); there the operator oracle is the
definition.  GPU tier: every case prints error / bound before it asserts.
"""
import ctypes

import numpy as np
import pytest

import aa_scenes as S
import depth_oracle as D
import silhouette_oracle as O
from oracle import raster_oracle as R

GRAD_TOL = 2e-5       # of the largest entry: what tests/test_raster.py holds fp32 atomics in arbitrary order to
UPSTREAM = 2000.0


def _checker_sheet(views=3):
    return S.merge(O.sparse_checker(33, 50, 27, 3, 6, 47, views=views), S.open_sheet(33, 50, views=views, box=(2, -1, 48, 25)))


def _backdrop_sheet():
    return S.merge(S.backdrop(32, 32), S.open_sheet(32, 32, nu=9, nv=8, views=1))


def _shifted_backdrop(views=5):
    pos, tri = S.backdrop(8, 8, views=views)
    pos = pos.copy()
    for b in range(views):                                        # every view sees the two triangles elsewhere (still over the whole image)
        pos[b, :, 0] += np.float32(0.011 * b)
        pos[b, :, 1] -= np.float32(0.007 * b)
    return pos, tri


def _one_triangle_views(H=6, W=8, views=5):
    """One triangle over the whole image in every view, each view's positions shifted: H W = 48 is no multiple of 64, so a wave of
    64 consecutive pixels holds the end of one view and the start of the next, both showing triangle 0."""
    pos = S._clip([-2.0, 3.0 * W, -2.0], [-2.0, -2.0, 3.0 * H], 0.5, H, W)
    pos = np.repeat(pos[None], views, axis=0).astype(np.float32)
    for b in range(views):
        pos[b, :, 0] += np.float32(0.05 * b)
        pos[b, :, 1] -= np.float32(0.03 * b)
    return pos, np.array([[0, 1, 2]], dtype=np.int32)


def _pairs_across_views_in_one_wave(ids, mask, hw):
    """Adjacent pixels of the flattened batch that lie in two views, show the same triangle, are both in the loss and fall into the
    same group of 64 (one wave of the backward kernel: one lane per pixel, in order)."""
    ids, m = np.asarray(ids).reshape(-1), np.asarray(mask).reshape(-1) != 0
    k = np.arange(hw, len(ids), hw)                                # first pixel of every view but the first
    return int(((ids[k] == ids[k - 1]) & (ids[k] > 0) & m[k] & m[k - 1] & (k // 64 == (k - 1) // 64)).sum())


SCENES = {
    "checker_sheet": (_checker_sheet, (33, 50)),
    "soup": (lambda: S.soup(48, 64), (48, 64)),
    "backdrop_views": (_shifted_backdrop, (8, 8)),
    "backdrop_sheet": (_backdrop_sheet, (32, 32)),
    "one_triangle_views": (_one_triangle_views, (6, 8)),
}


def _inputs(B, V, res, seed=11):
    """Random world positions, cameras in [2, 3]^3, targets in [2, 4], a mask with about 30 % zeros (float32)."""
    rng = np.random.default_rng(seed)
    H, W = res
    world = rng.standard_normal((V, 3)).astype(np.float32)
    campos = rng.uniform(2.0, 3.0, (B, 3)).astype(np.float32)
    target = rng.uniform(2.0, 4.0, (B, H, W)).astype(np.float32)
    mask = (rng.uniform(0.5, 1.5, (B, H, W)) * (rng.random((B, H, W)) > 0.3)).astype(np.float32)
    return world, campos, target, mask


# ================================================================ CPU tier ================================================================

def test_depth_abi_rejects_bad_arguments():
    """The entry points check their arguments before any device call (this test runs without a GPU): negative sizes, every null
    pointer by its name; tsamd_depth_mse_workspace_bytes is monotone, 256-byte aligned and -1 on a negative count."""
    from tssplat_amd import _capi
    lib = _capi.load()
    p = ctypes.c_void_p(256)                                       # a non-null pointer that is never dereferenced: every call below fails first

    def err(rc):
        assert rc != 0
        return lib.tsamd_last_error().decode()

    def fwd(batch=1, V=3, T=1, H=8, W=8, pos=p, tri=p, ids=p, world=p, campos=p, target=p, mask=p, ws=p, loss=p, d=p):
        return lib.tsamd_depth_mse(pos, batch, V, tri, T, H, W, ids, world, campos, target, mask, ws, loss, d, None)

    def bwd(batch=1, V=3, T=1, H=8, W=8, pos=p, tri=p, ids=p, world=p, campos=p, target=p, mask=p, gl=p, acc=0, gw=p, gp=p):
        return lib.tsamd_depth_mse_backward(pos, batch, V, tri, T, H, W, ids, world, campos, target, mask, gl, acc, gw, gp, None)

    shared = (("pos", "pos_clip_dev"), ("tri", "tri_dev"), ("ids", "ids_dev"), ("world", "world_pos_dev"), ("campos", "campos_dev"),
              ("target", "target_dev"), ("mask", "mask_dev"))
    for call in (fwd, bwd):
        for kw in ({"H": 8193}, {"W": 8193}, {"batch": -1}, {"H": -1}, {"W": -1}):
            assert "out of range (0 .. 8192 pixels per side)" in err(call(**kw)), (call.__name__, kw)
        for kw in ({"T": 1 << 24}, {"T": -1}, {"V": -1}):
            assert "2^24 - 1 triangles" in err(call(**kw)), (call.__name__, kw)
        for name, word in shared:
            assert err(call(**{name: None})).endswith(word + " is null"), (call.__name__, name)
    for name, word in (("ws", "workspace_dev"), ("loss", "loss_out_dev")):
        assert err(fwd(**{name: None})).endswith(word + " is null")
    assert err(fwd(H=0, loss=None)).endswith("loss_out_dev is null")                 # (the loss is stored even of nothing)
    for name, word in (("gl", "grad_loss_dev"), ("gw", "grad_world_dev"), ("gp", "grad_pos_dev")):
        assert err(bwd(**{name: None})).endswith(word + " is null")
    assert lib.tsamd_depth_mse_workspace_bytes(-1) == -1
    sizes = [0, 1, 3, 4, 1023, 1024, 1025, 4950, 1 << 20, (1 << 20) + 1, 120 * 512 * 512, 1 << 33]
    got = [lib.tsamd_depth_mse_workspace_bytes(n) for n in sizes]
    assert all(b > 0 and b % 256 == 0 for b in got) and got == sorted(got) and got[-1] > got[0]


@pytest.mark.parametrize("scene", ["backdrop_sheet", "backdrop_views", "soup"])
def test_oracle_grad_world_agrees_with_central_differences(scene):
    """With the ids (the whole ``rast`` image) frozen the loss is a smooth function of ``world_pos`` (d stays near 2 .. 6, far from
    the kink of the norm), so ``grad_world`` must agree with central differences in float64.  Step h = 1e-5 on entries of size 1:
    truncation h^2 |f'''| / 6 ~ 1e-11 |f'''|, cancellation 2^-53 |loss| / h ~ 1e-11 |loss| -- with the loss and its derivatives of
    order 1 .. 100 here (times the upstream 2 000), both stay below 1e-8 of a largest entry of several hundred; a factor of ten is
    left for third derivatives larger than estimated (grazing views of the soup): the bound is 1e-7 of the largest entry."""
    build, res = SCENES[scene]
    pos, tri = build()
    B, V = pos.shape[:2]
    world, campos, target, mask = _inputs(B, V, res)
    rast = R.rasterize(pos, tri, res)
    covered = rast[..., 3] > 0
    assert (covered & (mask != 0)).sum() >= 50
    grad_world, grad_pos = D.backward(rast, pos, tri, world, campos, target, mask, UPSTREAM)
    assert grad_world.shape == (V, 3) and grad_pos.shape == (B, V, 4)
    h = 1e-5
    w64 = world.astype(np.float64)
    fd = np.zeros_like(w64)
    for i in range(V):
        for c in range(3):
            up, dn = w64.copy(), w64.copy()
            up[i, c] += h
            dn[i, c] -= h
            fd[i, c] = UPSTREAM * (D.loss(rast, tri, up, campos, target, mask) - D.loss(rast, tri, dn, campos, target, mask)) / (2 * h)
    scale = np.abs(grad_world).max()
    err = np.abs(grad_world - fd).max()
    print(f"{scene}: |grad_world| max {scale:.3e}, against central differences {err:.3e} ({err / scale:.2e} of the largest entry)")
    assert scale > 0 and err <= 1e-7 * scale
    assert np.abs(grad_pos).max() > 0 and np.all(grad_pos[..., 2] == 0.0)            # z carries no gradient


# ================================================================ GPU tier ================================================================

class _Device:
    """One scene on the device, driven through the C ABI: tsamd_silhouette for the ids, then tsamd_depth_mse / _backward."""

    def __init__(self, pos_np, tri_np, res):
        import torch
        import tssplat_amd.dr as dr
        from tssplat_amd import _capi
        self.torch, self.capi, self.lib = torch, _capi, _capi.load()
        self.H, self.W = res
        self.pos = torch.from_numpy(np.ascontiguousarray(pos_np)).cuda()
        self.tri = torch.from_numpy(np.ascontiguousarray(tri_np)).cuda()
        self.B, self.V, self.T = int(self.pos.shape[0]), int(self.pos.shape[1]), int(self.tri.shape[0])
        ctx = dr.RasterizeCudaContext()
        self.rast = dr.rasterize(ctx, self.pos, self.tri, resolution=[self.H, self.W], grad_db=False)[0].cpu().numpy()
        topo = dr.antialias_construct_topology_hash(self.tri)
        lib = self.lib
        ws = torch.empty(max(lib.tsamd_rasterize_workspace_bytes(self.B, self.V, self.H, self.W), 8), dtype=torch.uint8, device="cuda")
        self.ids = torch.empty((self.B, self.H, self.W), dtype=torch.int32, device="cuda")
        masks = torch.empty(max(lib.tsamd_pair_masks_bytes(self.B, self.H, self.W), 8), dtype=torch.uint8, device="cuda")
        alpha = torch.empty((self.B, self.H, self.W, 1), device="cuda")
        _capi.check(lib.tsamd_silhouette(self.pos.data_ptr(), self.B, self.V, self.tri.data_ptr(), self.T, topo.opp.data_ptr(), self.H, self.W, ws.data_ptr(),
                                         self.ids.data_ptr(), masks.data_ptr(), alpha.data_ptr(), None))
        torch.cuda.synchronize()
        assert np.array_equal(self.ids.cpu().numpy(), self.rast[..., 3].astype(np.int32))

    def put(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def forward(self, world, campos, target, mask, ids=None, want_d=True):
        """(loss as a one-element float32 tensor, d[B, H, W] numpy or None)"""
        torch, lib = self.torch, self.lib
        n = self.B * self.H * self.W
        ws = torch.empty(lib.tsamd_depth_mse_workspace_bytes(n), dtype=torch.uint8, device="cuda")
        loss = torch.full((1,), -3.0, device="cuda")
        d = torch.full((self.B, self.H, self.W), -7.0, device="cuda") if want_d else None
        args = [self.put(k) for k in (world, campos, target, mask)]
        ids = self.ids if ids is None else ids
        self.capi.check(lib.tsamd_depth_mse(self.pos.data_ptr(), self.B, self.V, self.tri.data_ptr(), self.T, self.H, self.W, ids.data_ptr(), *(a.data_ptr() for a in args),
                                            ws.data_ptr(), loss.data_ptr(), d.data_ptr() if want_d else None, None))
        torch.cuda.synchronize()
        return loss, (d.cpu().numpy() if want_d else None)

    def backward(self, world, campos, target, mask, upstream=UPSTREAM, accumulate=0, prefill=None, ids=None):
        """(grad_world[V, 3], grad_pos[B, V, 4]) as numpy; ``prefill``: what grad_pos holds before the call (default: NaN)"""
        torch, lib = self.torch, self.lib
        args = [self.put(k) for k in (world, campos, target, mask)]
        gl = torch.tensor([upstream], dtype=torch.float32, device="cuda")
        gw = torch.full((self.V, 3), float("nan"), device="cuda")
        gp = torch.full((self.B, self.V, 4), float("nan"), device="cuda") if prefill is None else self.put(prefill).clone()
        ids = self.ids if ids is None else ids
        self.capi.check(lib.tsamd_depth_mse_backward(self.pos.data_ptr(), self.B, self.V, self.tri.data_ptr(), self.T, self.H, self.W, ids.data_ptr(),
                                                     *(a.data_ptr() for a in args), gl.data_ptr(), accumulate, gw.data_ptr(), gp.data_ptr(), None))
        torch.cuda.synchronize()
        return gw.cpu().numpy(), gp.cpu().numpy()


def _bits(t):
    import torch
    return int(t.reshape(1).view(torch.int32).item())


def _check_gradients(label, got_world, got_pos, want_world, want_pos):
    sw, sp = np.abs(want_world).max(), np.abs(want_pos).max()
    ew, ep = np.abs(got_world - want_world).max(), np.abs(got_pos - want_pos).max()
    print(f"{label}: grad_world max {sw:.3e} error {ew:.3e} ({ew / sw / GRAD_TOL:.3f} of the bound); grad_pos max {sp:.3e} error {ep:.3e} "
          f"({ep / sp / GRAD_TOL:.3f} of the bound)")
    assert sw > 0 and sp > 0
    assert np.isfinite(got_world).all() and np.isfinite(got_pos).all()
    assert ew <= GRAD_TOL * sw and ep <= GRAD_TOL * sp
    assert np.abs(got_world).max() > 0 and np.abs(got_pos).max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["checker_sheet", "soup"])
def test_depth_value_image_repeatability_and_backward(scene):
    """3 x 33 x 50 (n = 4 950: no multiple of 4 / 64 / 256, views end inside a chunk) and the 2 x 48 x 64 soup (sub-pixel triangles:
    the no-run path; vertices at w <= 0; a NaN vertex whose triangles are dropped; perspective w): d and the loss within the two
    bounds of tests/depth_oracle.py, two calls with equal loss bits, both gradients (upstream 2 000) against the oracle fed with
    the GPU's own rast."""
    build, res = SCENES[scene]
    pos, tri = build()
    dev = _Device(pos, tri, res)
    B, V = pos.shape[:2]
    world, campos, target, mask = _inputs(B, V, res)
    covered = dev.rast[..., 3] > 0
    assert ((~covered) & (mask != 0)).sum() >= 20                  # the || campos || term is in the loss
    assert (covered & (mask != 0)).sum() >= 200 and (covered & (mask == 0)).sum() >= 50
    if scene == "checker_sheet":
        assert (B * res[0] * res[1]) % 4 != 0 and (res[0] * res[1]) % 64 != 0
    loss, d = dev.forward(world, campos, target, mask)
    d64, d_bound = D.depth_bound(dev.rast, tri, world, campos)
    ratio_d = float(np.max(np.abs(d.astype(np.float64) - d64) / d_bound))
    want, l_bound = D.loss_bound(d, target, mask)
    ratio_l = abs(float(loss) - want) / l_bound
    print(f"{scene}: d error / bound {ratio_d:.3f}; loss {float(loss):.9g} against {want:.12g}, error / bound {ratio_l:.3f}")
    assert np.all(np.abs(d.astype(np.float64) - d64) <= d_bound)
    to_camera = np.broadcast_to(np.linalg.norm(campos.astype(np.float64), axis=1)[:, None, None], d.shape)
    assert np.array_equal(d64[~covered], to_camera[~covered])      # background: x = 0
    assert want > 0 and abs(float(loss) - want) <= l_bound
    again, _ = dev.forward(world, campos, target, mask)
    no_image, none = dev.forward(world, campos, target, mask, want_d=False)
    assert none is None and _bits(loss) == _bits(again) == _bits(no_image)
    gw, gp = dev.backward(world, campos, target, mask)
    want_w, want_p = D.backward(dev.rast, pos, tri, world, campos, target, mask, UPSTREAM)
    _check_gradients(scene, gw, gp, want_w, want_p)
    assert np.all(gp[..., 2] == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["backdrop_views", "one_triangle_views", "backdrop_sheet"])
def test_depth_backward_runs_within_and_across_views(scene):
    """5 views x 8 x 8 of a backdrop: the same two triangles in every view, runs 8 .. 64 lanes long (a view is exactly one wave there,
    so no run can cross into the next).  5 views x 6 x 8 of one triangle: every wave holds the end of one view and the start of the
    next on the same id, both in the loss -- a run key without the view adds one view's gradient to another's ``grad_pos``; the
    scene also takes the forward through its several-views-per-wave path (fewer than 256 pixels per view).  1 x 32 x 32 backdrop +
    sheet: long runs inside one view."""
    build, res = SCENES[scene]
    pos, tri = build()
    dev = _Device(pos, tri, res)
    B, V = pos.shape[:2]
    hw = res[0] * res[1]
    world, campos, target, mask = _inputs(B, V, res, seed=13)
    ids = dev.rast[..., 3].astype(np.int64).reshape(-1)
    assert (ids > 0).all()
    same = ids[1:] == ids[:-1]
    assert same.mean() > 0.5
    if scene == "backdrop_views":
        assert B * hw > 64 and hw == 64
        assert (ids.reshape(B, -1)[:-1, -1] == ids.reshape(B, -1)[1:, 0]).any()          # a view ends on the id the next one starts with
    if scene == "one_triangle_views":
        assert hw % 64 != 0 and hw < 256
        n_across = _pairs_across_views_in_one_wave(ids, mask, hw)
        print(f"{scene}: {n_across} same-id pairs across a view boundary inside one wave")
        assert n_across >= 2
        loss, d = dev.forward(world, campos, target, mask)
        d64, d_bound = D.depth_bound(dev.rast, tri, world, campos)
        want, l_bound = D.loss_bound(d, target, mask)
        print(f"{scene}: d error / bound {np.max(np.abs(d - d64) / d_bound):.3f}, loss error / bound {abs(float(loss) - want) / l_bound:.3f}")
        assert np.all(np.abs(d - d64) <= d_bound) and want > 0 and abs(float(loss) - want) <= l_bound
        per_view = np.linalg.norm((d64 - d64[:1]).reshape(B, -1), axis=1)
        assert np.all(per_view[1:] > 0)                                                  # (every view has its own camera and shift)
    gw, gp = dev.backward(world, campos, target, mask)
    want_w, want_p = D.backward(dev.rast, pos, tri, world, campos, target, mask, UPSTREAM)
    _check_gradients(scene, gw, gp, want_w, want_p)
    scale = np.abs(want_p).max()
    for b in range(B):
        err = np.abs(gp[b] - want_p[b]).max()
        print(f"{scene}: view {b} grad_pos error {err:.3e} ({err / scale / GRAD_TOL:.3f} of the bound)")
        assert err <= GRAD_TOL * scale and np.abs(want_p[b]).max() > 0


@pytest.mark.gpu
def test_depth_backward_accumulate_flag():
    """accumulate_pos = 1 on a pre-filled grad_pos gives pre-fill + depth gradient, 0 overwrites; grad_world is zero-filled either
    way (the two runs' atomics arrive in their own order: equal within the gradient bound)."""
    build, res = SCENES["checker_sheet"]
    pos, tri = build()
    dev = _Device(pos, tri, res)
    B, V = pos.shape[:2]
    world, campos, target, mask = _inputs(B, V, res, seed=17)
    prefill = np.random.default_rng(1).standard_normal((B, V, 4)).astype(np.float32)
    gw0, gp0 = dev.backward(world, campos, target, mask, accumulate=0, prefill=prefill)
    gw1, gp1 = dev.backward(world, campos, target, mask, accumulate=1, prefill=prefill)
    want_w, want_p = D.backward(dev.rast, pos, tri, world, campos, target, mask, UPSTREAM)
    _check_gradients("overwrite", gw0, gp0, want_w, want_p)
    _check_gradients("accumulate: grad_world", gw1, gp0, want_w, want_p)
    # the same grad_world either way (the atomics of two launches arrive in their own order: the same bound, not the same bits)
    assert np.abs(gw1 - gw0).max() <= GRAD_TOL * np.abs(want_w).max()
    scale = np.abs(want_p).max()
    err = np.abs(gp1.astype(np.float64) - (prefill.astype(np.float64) + want_p)).max()
    # one more float32 rounding per entry: the sum lands on a pre-fill of size <= max |prefill|
    tol = GRAD_TOL * scale + D.U * (np.abs(prefill).max() + scale)
    print(f"accumulate: error {err:.3e}, bound {tol:.3e}")
    assert err <= tol
    untouched = want_p == 0.0
    assert untouched.any() and np.array_equal(gp1[untouched], prefill[untouched]) and np.all(gp0[untouched] == 0.0)


@pytest.mark.gpu
def test_depth_degenerate_inputs():
    """Mask all zero; world = campos = 0 (d = 0 everywhere); no views, no pixels, no triangles; ids beyond the triangle list."""
    import torch
    from tssplat_amd import _capi
    build, res = SCENES["checker_sheet"]
    pos, tri = build()
    dev = _Device(pos, tri, res)
    B, V = pos.shape[:2]
    H, W = res
    world, campos, target, mask = _inputs(B, V, res, seed=19)
    # mask all zero
    loss, d = dev.forward(world, campos, target, np.zeros_like(mask))
    gw, gp = dev.backward(world, campos, target, np.zeros_like(mask))
    assert float(loss) == 0.0 and not gw.any() and not gp.any()
    d64, d_bound = D.depth_bound(dev.rast, tri, world, campos)
    assert np.all(np.abs(d - d64) <= d_bound)                      # (the image is still whole)
    # d = 0 everywhere
    loss, d = dev.forward(np.zeros_like(world), np.zeros_like(campos), target, mask)
    gw, gp = dev.backward(np.zeros_like(world), np.zeros_like(campos), target, mask)
    assert np.all(d == 0.0) and float(loss) > 0
    assert np.isfinite(gw).all() and np.isfinite(gp).all() and not gw.any() and not gp.any()
    # nothing to render: the loss is stored as 0 and nothing else is written
    lib = dev.lib
    p = dev.pos.data_ptr()
    for batch, h, w, T in ((0, H, W, dev.T), (B, 0, W, dev.T), (B, H, 0, dev.T), (B, H, W, 0)):
        out = torch.full((1,), 5.0, device="cuda")
        d_img = torch.full((B, H, W), -7.0, device="cuda")
        args = [dev.put(k) for k in (world, campos, target, mask)]
        ws = torch.empty(256, dtype=torch.uint8, device="cuda")
        _capi.check(lib.tsamd_depth_mse(p, batch, V, dev.tri.data_ptr(), T, h, w, dev.ids.data_ptr(), *(a.data_ptr() for a in args), ws.data_ptr(),
                                        out.data_ptr(), d_img.data_ptr(), None))
        gl = torch.tensor([UPSTREAM], device="cuda")
        gw_t = torch.full((V, 3), float("nan"), device="cuda")
        gp_t = torch.full((B, V, 4), float("nan"), device="cuda")
        _capi.check(lib.tsamd_depth_mse_backward(p, batch, V, dev.tri.data_ptr(), T, h, w, dev.ids.data_ptr(), *(a.data_ptr() for a in args), gl.data_ptr(), 0,
                                                 gw_t.data_ptr(), gp_t.data_ptr(), None))
        torch.cuda.synchronize()
        assert float(out) == 0.0 and bool((d_img == -7.0).all()), (batch, h, w, T)
        assert not bool(gw_t.any()) and not bool(gp_t[:batch].any()), (batch, h, w, T)
    out = torch.full((1,), 5.0, device="cuda")
    _capi.check(lib.tsamd_depth_mse(None, 0, 0, None, 0, 0, 0, None, None, None, None, None, None, out.data_ptr(), None, None))
    torch.cuda.synchronize()
    assert float(out) == 0.0
    # ids that name no triangle of the list behave as background
    ids = dev.ids.clone()
    flat = ids.view(-1)
    covered = torch.nonzero(flat > 0).view(-1)
    pick = covered[::3]
    assert pick.numel() >= 100
    foreign = flat.clone()
    foreign[pick[0::3]] = dev.T + 1
    foreign[pick[1::3]] = 2 ** 31 - 1
    foreign[pick[2::3]] = -5
    background = flat.clone()
    background[pick] = 0
    f_ids, b_ids = foreign.view_as(ids).contiguous(), background.view_as(ids).contiguous()
    loss_f, d_f = dev.forward(world, campos, target, mask, ids=f_ids)
    loss_b, d_b = dev.forward(world, campos, target, mask, ids=b_ids)
    assert _bits(loss_f) == _bits(loss_b) and np.array_equal(d_f, d_b)
    assert _bits(loss_f) != _bits(dev.forward(world, campos, target, mask)[0])
    gw_f, gp_f = dev.backward(world, campos, target, mask, ids=f_ids)
    gw_b, gp_b = dev.backward(world, campos, target, mask, ids=b_ids)
    _check_gradients("foreign ids", gw_f, gp_f, gw_b.astype(np.float64), gp_b.astype(np.float64))


def _chain(pos, tri, world, campos, res, target_alpha, target_depth, mask, weights):
    """The operator chain at the dr level: (alpha loss, depth loss, d) with ``weights[0] alpha + weights[1] depth`` backpropagated."""
    import torch
    import tssplat_amd.dr as dr
    ctx = dr.RasterizeCudaContext()
    rast, _ = dr.rasterize(ctx, pos, tri, resolution=list(res), grad_db=False)
    alpha = torch.clamp(rast[..., -1:].detach(), 0, 1).contiguous()
    alpha = dr.antialias(alpha, rast, pos, tri, topology_hash=None, pos_gradient_boost=1.0)
    alpha_loss = torch.nn.MSELoss()(alpha[..., -1], target_alpha)
    x, _ = dr.interpolate(world[None, ...], rast, tri)
    d = torch.norm(x - campos[:, None, None, :], dim=-1, keepdim=True)
    depth_loss = torch.nn.MSELoss()(d[..., -1] * mask, target_depth * mask)
    (weights[0] * alpha_loss + weights[1] * depth_loss).backward()
    return alpha_loss.detach(), depth_loss.detach(), d.detach()


@pytest.mark.gpu
def test_silhouette_depth_mse_against_the_operators():
    """dr.silhouette_depth_mse on the 33 x 50 scene against rasterize -> clamp -> antialias -> MSELoss plus interpolate -> norm ->
    masked MSELoss: alpha_loss has dr.silhouette_mse's bits, depth_loss is within the loss bound of the chain's own d evaluated in
    float64, pos.grad and world_pos.grad within 2e-5 of their largest entries; one autograd node."""
    import torch
    import tssplat_amd.dr as dr
    build, res = SCENES["checker_sheet"]
    pos_np, tri_np = build()
    B, V = pos_np.shape[:2]
    world_np, campos_np, target_np, mask_np = _inputs(B, V, res, seed=23)
    tri = torch.from_numpy(tri_np).cuda()
    campos, target_depth, mask = (torch.from_numpy(k).cuda() for k in (campos_np, target_np, mask_np))
    torch.manual_seed(5)
    target_alpha = torch.rand(B, *res, device="cuda")
    weights = (2000.0, 700.0)
    pos_c = torch.from_numpy(pos_np).cuda().requires_grad_(True)
    world_c = torch.from_numpy(world_np).cuda().requires_grad_(True)
    _, _, d_chain = _chain(pos_c, tri, world_c, campos, res, target_alpha, target_depth, mask, weights)
    pos = torch.from_numpy(pos_np).cuda().requires_grad_(True)
    world = torch.from_numpy(world_np).cuda().requires_grad_(True)
    ctx = dr.RasterizeCudaContext()
    alpha_loss, depth_loss, alpha, d = dr.silhouette_depth_mse(ctx, pos, tri, list(res), target_alpha, world, campos, target_depth[..., None], mask,
                                                               return_images=True)
    assert alpha_loss.dim() == 0 and depth_loss.dim() == 0 and alpha.shape == d.shape == (B,) + res + (1,)
    assert not alpha.requires_grad and not d.requires_grad and alpha_loss.grad_fn is depth_loss.grad_fn
    pair = dr.silhouette_depth_mse(ctx, pos, tri, list(res), target_alpha, world[None], campos, target_depth, mask[..., None])
    assert len(pair) == 2 and _bits(pair[0].detach()) == _bits(alpha_loss.detach()) and _bits(pair[1].detach()) == _bits(depth_loss.detach())
    alone = dr.silhouette_mse(ctx, pos.detach(), tri, list(res), target_alpha)
    assert _bits(alone) == _bits(alpha_loss.detach())
    want, bound = D.loss_bound(d_chain.cpu().numpy()[..., 0], target_np, mask_np)
    got = float(depth_loss.detach())
    print(f"dr: depth_loss {got:.9g} against the chain in float64 {want:.12g}, error / bound {abs(got - want) / bound:.3f}; "
          f"d against the chain's {float((d - d_chain).abs().max()):.3e}")
    assert want > 0 and abs(got - want) <= bound
    (weights[0] * alpha_loss + weights[1] * depth_loss).backward()
    for label, got_g, want_g in (("pos.grad", pos.grad, pos_c.grad), ("world_pos.grad", world.grad, world_c.grad)):
        scale = float(want_g.abs().max())
        err = float((got_g - want_g).abs().max())
        print(f"dr: {label} max {scale:.3e}, error {err:.3e} ({err / scale / GRAD_TOL:.3f} of the bound)")
        assert scale > 0 and err <= GRAD_TOL * scale
    with pytest.raises(RuntimeError, match="world_pos must be"):
        dr.silhouette_depth_mse(ctx, pos, tri, list(res), target_alpha, world[:-1], campos, target_depth, mask)
    with pytest.raises(RuntimeError, match="campos must be"):
        dr.silhouette_depth_mse(ctx, pos, tri, list(res), target_alpha, world, campos[:-1], target_depth, mask)
    with pytest.raises(RuntimeError, match="depth_mask must be"):
        dr.silhouette_depth_mse(ctx, pos, tri, list(res), target_alpha, world, campos, target_depth, mask[:, :-1])


@pytest.mark.gpu
def test_renderer_silhouette_depth_loss(aveg):
    """MeshRasterizer.silhouette_depth_loss on the golden mesh, 2 views x 64^2, against the default forward(only_alpha=True,
    fit_depth=True) and the trainer's two MSELoss calls: both losses within their bounds (the alpha loss: 4 * 2^-24 L, as
    tests/test_silhouette.py derives it), ``d`` within the d bound of out["d"], ``shaded`` within 2e-6, ``tet_v.grad`` of
    (20 img + 100 depth) 100 + reg within 2e-5 of its largest entry; depth_mask=None is depth_mask=target_alpha."""
    import types
    import torch
    from tssplat_amd import geometry, renderers
    flags = types.SimpleNamespace(smooth_eng_coeff=2e-4, barrier_coeff=2e-4, increase_order_iter=1000)
    rest, tets = aveg
    geo = geometry.TetMeshGeometry(rest, tets, smooth_barrier_param=flags)
    ren = renderers.MeshRasterizer(geo)
    mvp = torch.from_numpy(R.orbit_mvps(2)).cuda()
    campos = torch.tensor([[0.0, 1.0, 3.0], [0.5, 1.0, -3.0]], device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(2)
    target_alpha = torch.rand(2, 64, 64, device="cuda", generator=gen)
    target_depth = torch.rand(2, 64, 64, device="cuda", generator=gen) * 2 + 2
    mse = torch.nn.MSELoss()

    geo.tet_v.grad = None
    out = ren(mvp, only_alpha=True, iter_num=5, resolution=64, fit_depth=True, campos=campos)
    img = mse(out["shaded"][..., -1], target_alpha) * 20
    img = img + mse(out["d"][..., -1] * target_alpha, target_depth * target_alpha) * 100
    (img * 100 + out["geo_regularization"]).backward()
    want_grad = geo.tet_v.grad.clone()
    frac = float((out["shaded"] > 0.5).float().mean())
    assert 0.05 < frac < 0.95

    geo.tet_v.grad = None
    got = ren.silhouette_depth_loss(mvp, target_alpha, campos, target_depth, iter_num=5, resolution=64)
    assert set(got) == {"img_loss", "depth_loss", "geo_regularization", "shaded", "d"}
    assert got["img_loss"].dim() == 0 and got["depth_loss"].dim() == 0 and not got["shaded"].requires_grad and not got["d"].requires_grad
    ((got["img_loss"] * 20 + got["depth_loss"] * 100) * 100 + got["geo_regularization"]).backward()
    got_grad = geo.tet_v.grad.clone()

    want_img = float(mse(out["shaded"][..., -1].detach().double(), target_alpha.double()))
    img_loss = float(got["img_loss"].detach())
    want_depth, depth_bound = D.loss_bound(out["d"].detach().cpu().numpy()[..., 0], target_depth.cpu().numpy(), target_alpha.cpu().numpy())
    depth_loss = float(got["depth_loss"].detach())
    print(f"renderer: img_loss error / bound {abs(img_loss - want_img) / (4 * D.U * want_img):.3f}, depth_loss {depth_loss:.9g} against {want_depth:.12g}, "
          f"error / bound {abs(depth_loss - want_depth) / depth_bound:.3f}")
    assert abs(img_loss - want_img) <= 4 * D.U * want_img
    assert want_depth > 0 and abs(depth_loss - want_depth) <= depth_bound
    assert float((got["shaded"] - out["shaded"].detach()).abs().max()) <= 2e-6
    # d against its own float64 evaluation, and against out["d"] (another float32 evaluation of the same expression)
    with torch.no_grad():
        data = geo(iter_num=5)
        pos_clip = ren.transform_pos(mvp, data.v_pos).contiguous()
        import tssplat_amd.dr as dr
        rast, _ = dr.rasterize(ren.glctx, pos_clip, data.t_pos_idx, resolution=[64, 64], grad_db=False)
    d64, d_bound = D.depth_bound(rast.cpu().numpy(), data.t_pos_idx.cpu().numpy(), data.v_pos.cpu().numpy(), campos.cpu().numpy())
    d_got = got["d"].cpu().numpy()[..., 0].astype(np.float64)
    d_chain = out["d"].detach().cpu().numpy()[..., 0].astype(np.float64)
    print(f"renderer: d error / bound {np.max(np.abs(d_got - d64) / d_bound):.3f} (against float64) {np.max(np.abs(d_got - d_chain) / d_bound):.3f} (against out['d'])")
    assert np.all(np.abs(d_got - d64) <= d_bound) and np.all(np.abs(d_got - d_chain) <= d_bound)
    scale = float(want_grad.abs().max())
    err = float((got_grad - want_grad).abs().max())
    print(f"renderer: tet_v.grad max {scale:.3e}, fused against the chain {err:.3e} ({err / scale / GRAD_TOL:.3f} of the bound)")
    assert scale > 0 and err <= GRAD_TOL * scale
    same = ren.silhouette_depth_loss(mvp, target_alpha, campos, target_depth, iter_num=5, resolution=64, depth_mask=target_alpha)
    assert _bits(same["depth_loss"].detach()) == _bits(got["depth_loss"].detach()) and _bits(same["img_loss"].detach()) == _bits(got["img_loss"].detach())
    assert torch.equal(same["d"], got["d"])
