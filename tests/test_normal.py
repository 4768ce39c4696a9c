"""The normal term without an image chain: tsamd_normal_mse / tsamd_normal_mse_backward, dr.silhouette_normal_mse and
MeshRasterizer.silhouette_normal_loss against the operator chain (rasterize -> interpolate -> masked MSELoss) and its float64
restatement (tests/normal_oracle.py over oracle/raster_oracle.py).

The scenes, the mask generator and the device harness are those of tests/test_depth.py (imported, not copied).  CPU tier: the
argument checks of the C ABI, and the oracle's own ``grad_attr`` against central differences (ids frozen); the clip positions are
not finite-differenced, for the reason test_depth.py gives.  GPU tier: every case prints error / bound before it asserts.

Preconditions: the cases on ``checker_sheet`` and ``soup`` assert at least 200 covered pixels in the loss, 50 covered pixels masked
out and 20 background pixels in the loss.  The run cases are backdrops -- every pixel covered, by construction -- and assert that
instead, with the run structure they are there for.
"""
import ctypes

import numpy as np
import pytest

import depth_oracle as D
import normal_oracle as N
import test_depth as TD
from oracle import raster_oracle as R

GRAD_TOL = TD.GRAD_TOL     # 2e-5 of the largest entry: what tests/test_raster.py holds fp32 atomics in arbitrary order to
UPSTREAM = 2000.0
SCENES = TD.SCENES
_bits = TD._bits


def _inputs(B, V, res, seed=11):
    """Random attr ~ N(0, 1), targets uniform in [-1, 1]^3, the mask of test_depth._inputs: about 30 % zeros, else in [0.5, 1.5]."""
    rng = np.random.default_rng(seed)
    H, W = res
    attr = rng.standard_normal((V, 3)).astype(np.float32)
    target = rng.uniform(-1.0, 1.0, (B, H, W, 3)).astype(np.float32)
    mask = (rng.uniform(0.5, 1.5, (B, H, W)) * (rng.random((B, H, W)) > 0.3)).astype(np.float32)
    return attr, target, mask


def _assert_mixed(covered, mask):
    """Covered pixels in the loss, covered pixels masked out, background pixels in the loss: all three paths are taken."""
    assert (covered & (mask != 0)).sum() >= 200 and (covered & (mask == 0)).sum() >= 50 and ((~covered) & (mask != 0)).sum() >= 20


# ================================================================ CPU tier ================================================================

def test_normal_abi_rejects_bad_arguments():
    """The entry points check their arguments before any device call (this test runs without a GPU): negative sizes, every null
    pointer by its name; tsamd_normal_mse_workspace_bytes is monotone, 256-byte aligned and -1 on a negative count."""
    from tssplat_amd import _capi
    lib = _capi.load()
    p = ctypes.c_void_p(256)                                       # a non-null pointer that is never dereferenced: every call below fails first

    def err(rc):
        assert rc != 0
        return lib.tsamd_last_error().decode()

    def fwd(batch=1, V=3, T=1, H=8, W=8, pos=p, tri=p, ids=p, attr=p, target=p, mask=p, ws=p, loss=p, n=p):
        return lib.tsamd_normal_mse(pos, batch, V, tri, T, H, W, ids, attr, target, mask, ws, loss, n, None)

    def bwd(batch=1, V=3, T=1, H=8, W=8, pos=p, tri=p, ids=p, attr=p, target=p, mask=p, gl=p, acc=0, ga=p, gp=p):
        return lib.tsamd_normal_mse_backward(pos, batch, V, tri, T, H, W, ids, attr, target, mask, gl, acc, ga, gp, None)

    shared = (("pos", "pos_clip_dev"), ("tri", "tri_dev"), ("ids", "ids_dev"), ("attr", "attr_dev"), ("target", "target_dev"), ("mask", "mask_dev"))
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
    for name, word in (("gl", "grad_loss_dev"), ("ga", "grad_attr_dev"), ("gp", "grad_pos_dev")):
        assert err(bwd(**{name: None})).endswith(word + " is null")
    assert lib.tsamd_normal_mse_workspace_bytes(-1) == -1
    sizes = [0, 1, 3, 4, 1023, 1024, 1025, 4950, 1 << 20, (1 << 20) + 1, 120 * 512 * 512, 1 << 33]
    got = [lib.tsamd_normal_mse_workspace_bytes(n) for n in sizes]
    assert all(b > 0 and b % 256 == 0 for b in got) and got == sorted(got) and got[-1] > got[0]


@pytest.mark.parametrize("scene", ["backdrop_sheet", "backdrop_views", "soup"])
def test_oracle_grad_attr_agrees_with_central_differences(scene):
    """With the ids (the whole ``rast`` image) frozen the loss is a QUADRATIC function of ``attr`` (n is linear in it), so a central
    difference has no truncation error at all; what is left is cancellation, 2^-53 |upstream loss| / h.  With h = 1e-5, the upstream
    2 000 and a loss of order 1 (attr ~ N(0, 1), targets in [-1, 1], masks <= 1.5) that is ~2e-8, against largest entries of order
    10 .. 100 (a vertex collects 2 000 * 2 x m u / (3 B H W) from tens to hundreds of pixels): below 1e-8 of the largest entry.  The
    bound is the one tests/test_depth.py derives for the same step size, 1e-7 of the largest entry -- its factor of ten for third
    derivatives is not needed here and is spent on nothing."""
    build, res = SCENES[scene]
    pos, tri = build()
    B, V = pos.shape[:2]
    attr, target, mask = _inputs(B, V, res)
    rast = R.rasterize(pos, tri, res)
    covered = rast[..., 3] > 0
    assert (covered & (mask != 0)).sum() >= 50
    grad_attr, grad_pos = N.backward(rast, pos, tri, attr, target, mask, UPSTREAM)
    assert grad_attr.shape == (V, 3) and grad_pos.shape == (B, V, 4)
    h = 1e-5
    a64 = attr.astype(np.float64)
    fd = np.zeros_like(a64)
    for i in range(V):
        for c in range(3):
            up, dn = a64.copy(), a64.copy()
            up[i, c] += h
            dn[i, c] -= h
            fd[i, c] = UPSTREAM * (N.loss(rast, tri, up, target, mask) - N.loss(rast, tri, dn, target, mask)) / (2 * h)
    scale = np.abs(grad_attr).max()
    err = np.abs(grad_attr - fd).max()
    print(f"{scene}: |grad_attr| max {scale:.3e}, against central differences {err:.3e} ({err / scale:.2e} of the largest entry)")
    assert scale > 0 and err <= 1e-7 * scale
    assert np.abs(grad_pos).max() > 0 and np.all(grad_pos[..., 2] == 0.0)            # z carries no gradient


# ================================================================ GPU tier ================================================================

class _Device(TD._Device):
    """test_depth's scene on the device (tsamd_silhouette for the ids, dr.rasterize for ``rast``), driven through tsamd_normal_mse*."""

    def forward(self, attr, target, mask, ids=None, want_n=True):
        """(loss as a one-element float32 tensor, n[B, H, W, 3] numpy or None)"""
        torch, lib = self.torch, self.lib
        ws = torch.empty(lib.tsamd_normal_mse_workspace_bytes(self.B * self.H * self.W), dtype=torch.uint8, device="cuda")
        loss = torch.full((1,), -3.0, device="cuda")
        n = torch.full((self.B, self.H, self.W, 3), -7.0, device="cuda") if want_n else None
        args = [self.put(k) for k in (attr, target, mask)]
        ids = self.ids if ids is None else ids
        self.capi.check(lib.tsamd_normal_mse(self.pos.data_ptr(), self.B, self.V, self.tri.data_ptr(), self.T, self.H, self.W, ids.data_ptr(),
                                             *(a.data_ptr() for a in args), ws.data_ptr(), loss.data_ptr(), n.data_ptr() if want_n else None, None))
        torch.cuda.synchronize()
        return loss, (n.cpu().numpy() if want_n else None)

    def backward(self, attr, target, mask, upstream=UPSTREAM, accumulate=0, prefill=None, ids=None):
        """(grad_attr[V, 3], grad_pos[B, V, 4]) as numpy; ``prefill``: what grad_pos holds before the call (default: NaN)"""
        torch, lib = self.torch, self.lib
        args = [self.put(k) for k in (attr, target, mask)]
        gl = torch.tensor([upstream], dtype=torch.float32, device="cuda")
        ga = torch.full((self.V, 3), float("nan"), device="cuda")
        gp = torch.full((self.B, self.V, 4), float("nan"), device="cuda") if prefill is None else self.put(prefill).clone()
        ids = self.ids if ids is None else ids
        self.capi.check(lib.tsamd_normal_mse_backward(self.pos.data_ptr(), self.B, self.V, self.tri.data_ptr(), self.T, self.H, self.W, ids.data_ptr(),
                                                      *(a.data_ptr() for a in args), gl.data_ptr(), accumulate, ga.data_ptr(), gp.data_ptr(), None))
        torch.cuda.synchronize()
        return ga.cpu().numpy(), gp.cpu().numpy()


def _check_gradients(label, got_attr, got_pos, want_attr, want_pos):
    sa, sp = np.abs(want_attr).max(), np.abs(want_pos).max()
    ea, ep = np.abs(got_attr - want_attr).max(), np.abs(got_pos - want_pos).max()
    print(f"{label}: grad_attr max {sa:.3e} error {ea:.3e} ({ea / sa / GRAD_TOL:.3f} of the bound); grad_pos max {sp:.3e} error {ep:.3e} "
          f"({ep / sp / GRAD_TOL:.3f} of the bound)")
    assert sa > 0 and sp > 0
    assert np.isfinite(got_attr).all() and np.isfinite(got_pos).all()
    assert ea <= GRAD_TOL * sa and ep <= GRAD_TOL * sp
    assert np.abs(got_attr).max() > 0 and np.abs(got_pos).max() > 0


def _check_image_and_loss(label, dev, tri, attr, target, mask, loss, n):
    """n within the per-component bound everywhere and exactly 0 on background, the loss within its bound"""
    n64, n_bound = N.normal_bound(dev.rast, tri, attr)
    err = np.abs(n.astype(np.float64) - n64)
    want, l_bound = N.loss_bound(n, target, mask)
    worst = float(np.max(err[n_bound > 0] / n_bound[n_bound > 0]))
    print(f"{label}: n error / bound {worst:.3f}; loss {float(loss):.9g} against {want:.12g}, error / bound {abs(float(loss) - want) / l_bound:.3f}")
    assert np.all(err <= n_bound)
    covered = dev.rast[..., 3] > 0
    assert np.all(n[~covered] == 0.0) and np.abs(n[covered]).max() > 0
    assert want > 0 and abs(float(loss) - want) <= l_bound


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["checker_sheet", "soup"])
def test_normal_value_image_repeatability_and_backward(scene):
    """3 x 33 x 50 (n = 4 950: no multiple of 4 / 64 / 256, views end inside a chunk) and the 2 x 48 x 64 soup (sub-pixel triangles:
    the no-run path; vertices at w <= 0; a NaN vertex whose triangles are dropped; perspective w): n and the loss within the two
    bounds of tests/normal_oracle.py, n exactly 0 on background, equal loss bits across two calls and with and without the image,
    both gradients (upstream 2 000) against the oracle fed with the GPU's own rast."""
    build, res = SCENES[scene]
    pos, tri = build()
    dev = _Device(pos, tri, res)
    B, V = pos.shape[:2]
    attr, target, mask = _inputs(B, V, res)
    _assert_mixed(dev.rast[..., 3] > 0, mask)
    if scene == "checker_sheet":
        assert (B * res[0] * res[1]) % 4 != 0 and (res[0] * res[1]) % 64 != 0
    loss, n = dev.forward(attr, target, mask)
    _check_image_and_loss(scene, dev, tri, attr, target, mask, loss, n)
    again, _ = dev.forward(attr, target, mask)
    no_image, none = dev.forward(attr, target, mask, want_n=False)
    assert none is None and _bits(loss) == _bits(again) == _bits(no_image)
    ga, gp = dev.backward(attr, target, mask)
    want_a, want_p = N.backward(dev.rast, pos, tri, attr, target, mask, UPSTREAM)
    _check_gradients(scene, ga, gp, want_a, want_p)
    assert np.all(gp[..., 2] == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["backdrop_views", "one_triangle_views", "backdrop_sheet"])
def test_normal_backward_runs_within_and_across_views(scene):
    """5 views x 8 x 8 of a backdrop: the same two triangles in every view, runs 8 .. 64 lanes long, several views per workgroup.
    5 views x 6 x 8 of one triangle: every wave holds the end of one view and the start of the next on the same id, both in the
    loss -- a run key without the view adds one view's gradient to another's ``grad_pos``; the scene also takes the forward through
    its several-views-per-wave path (fewer than 256 pixels per view).  1 x 32 x 32 backdrop + sheet: long runs inside one view."""
    build, res = SCENES[scene]
    pos, tri = build()
    dev = _Device(pos, tri, res)
    B, V = pos.shape[:2]
    hw = res[0] * res[1]
    attr, target, mask = _inputs(B, V, res, seed=13)
    ids = dev.rast[..., 3].astype(np.int64).reshape(-1)
    assert (ids > 0).all() and (mask != 0).sum() >= 0.5 * mask.size and (mask == 0).sum() >= 0.1 * mask.size
    assert (ids[1:] == ids[:-1]).mean() > 0.5
    if scene == "backdrop_views":
        assert B * hw > 64 and hw == 64
        assert (ids.reshape(B, -1)[:-1, -1] == ids.reshape(B, -1)[1:, 0]).any()          # a view ends on the id the next one starts with
    if scene == "one_triangle_views":
        assert hw % 64 != 0 and hw < 256
        n_across = TD._pairs_across_views_in_one_wave(ids, mask, hw)
        print(f"{scene}: {n_across} same-id pairs across a view boundary inside one wave")
        assert n_across >= 1
        loss, n = dev.forward(attr, target, mask)
        _check_image_and_loss(scene, dev, tri, attr, target, mask, loss, n)
        per_view = np.linalg.norm((n - n[:1]).reshape(B, -1), axis=1)
        assert np.all(per_view[1:] > 0)                                                  # (every view has its own shift)
    ga, gp = dev.backward(attr, target, mask)
    want_a, want_p = N.backward(dev.rast, pos, tri, attr, target, mask, UPSTREAM)
    _check_gradients(scene, ga, gp, want_a, want_p)
    scale = np.abs(want_p).max()
    for b in range(B):
        err = np.abs(gp[b] - want_p[b]).max()
        print(f"{scene}: view {b} grad_pos error {err:.3e} ({err / scale / GRAD_TOL:.3f} of the bound)")
        assert err <= GRAD_TOL * scale and np.abs(want_p[b]).max() > 0


@pytest.mark.gpu
def test_normal_backward_accumulate_flag():
    """accumulate_pos = 1 on a pre-filled grad_pos gives pre-fill + normal gradient, 0 overwrites (a NaN pre-fill included);
    grad_attr is zero-filled either way (the two runs' atomics arrive in their own order: equal within the gradient bound)."""
    build, res = SCENES["checker_sheet"]
    pos, tri = build()
    dev = _Device(pos, tri, res)
    B, V = pos.shape[:2]
    attr, target, mask = _inputs(B, V, res, seed=17)
    _assert_mixed(dev.rast[..., 3] > 0, mask)
    prefill = np.random.default_rng(1).standard_normal((B, V, 4)).astype(np.float32)
    ga0, gp0 = dev.backward(attr, target, mask, accumulate=0, prefill=prefill)
    gan, gpn = dev.backward(attr, target, mask, accumulate=0)                          # grad_attr and grad_pos start as NaN
    ga1, gp1 = dev.backward(attr, target, mask, accumulate=1, prefill=prefill)          # grad_attr starts as NaN here too
    want_a, want_p = N.backward(dev.rast, pos, tri, attr, target, mask, UPSTREAM)
    _check_gradients("overwrite", ga0, gp0, want_a, want_p)
    _check_gradients("overwrite NaN", gan, gpn, want_a, want_p)
    _check_gradients("accumulate: grad_attr", ga1, gp0, want_a, want_p)
    assert np.abs(ga1 - ga0).max() <= GRAD_TOL * np.abs(want_a).max()
    scale = np.abs(want_p).max()
    err = np.abs(gp1.astype(np.float64) - (prefill.astype(np.float64) + want_p)).max()
    # one more float32 rounding per entry: the sum lands on a pre-fill of size <= max |prefill|
    tol = GRAD_TOL * scale + D.U * (np.abs(prefill).max() + scale)
    print(f"accumulate: error {err:.3e}, bound {tol:.3e}")
    assert err <= tol
    untouched = want_p == 0.0
    assert untouched.any() and np.array_equal(gp1[untouched], prefill[untouched]) and np.all(gp0[untouched] == 0.0) and np.all(gpn[untouched] == 0.0)


@pytest.mark.gpu
def test_normal_degenerate_inputs():
    """Mask all zero; attr = 0; no views, no pixels, no triangles; ids that name no triangle of the list."""
    import torch
    from tssplat_amd import _capi
    build, res = SCENES["checker_sheet"]
    pos, tri = build()
    dev = _Device(pos, tri, res)
    B, V = pos.shape[:2]
    H, W = res
    attr, target, mask = _inputs(B, V, res, seed=19)
    _assert_mixed(dev.rast[..., 3] > 0, mask)
    # mask all zero
    loss, n = dev.forward(attr, target, np.zeros_like(mask))
    ga, gp = dev.backward(attr, target, np.zeros_like(mask))
    assert float(loss) == 0.0 and not ga.any() and not gp.any()
    n64, n_bound = N.normal_bound(dev.rast, tri, attr)
    assert np.all(np.abs(n - n64) <= n_bound) and np.abs(n).max() > 0                   # (the image is still whole)
    # attr = 0: n = 0 everywhere, the loss is the target's own, the gradients are finite
    loss, n = dev.forward(np.zeros_like(attr), target, mask)
    ga, gp = dev.backward(np.zeros_like(attr), target, mask)
    assert np.all(n == 0.0) and float(loss) > 0
    assert np.isfinite(ga).all() and np.isfinite(gp).all() and ga.any() and not gp.any()   # (du = dv = 0: every a0 - a2 is 0)
    # nothing to render: the loss is stored as 0 and nothing else is written
    lib = dev.lib
    p = dev.pos.data_ptr()
    for batch, h, w, T in ((0, H, W, dev.T), (B, 0, W, dev.T), (B, H, 0, dev.T), (B, H, W, 0)):
        out = torch.full((1,), 5.0, device="cuda")
        n_img = torch.full((B, H, W, 3), -7.0, device="cuda")
        args = [dev.put(k) for k in (attr, target, mask)]
        ws = torch.empty(256, dtype=torch.uint8, device="cuda")
        _capi.check(lib.tsamd_normal_mse(p, batch, V, dev.tri.data_ptr(), T, h, w, dev.ids.data_ptr(), *(a.data_ptr() for a in args), ws.data_ptr(),
                                         out.data_ptr(), n_img.data_ptr(), None))
        gl = torch.tensor([UPSTREAM], device="cuda")
        ga_t = torch.full((V, 3), float("nan"), device="cuda")
        gp_t = torch.full((B, V, 4), float("nan"), device="cuda")
        _capi.check(lib.tsamd_normal_mse_backward(p, batch, V, dev.tri.data_ptr(), T, h, w, dev.ids.data_ptr(), *(a.data_ptr() for a in args), gl.data_ptr(), 0,
                                                  ga_t.data_ptr(), gp_t.data_ptr(), None))
        torch.cuda.synchronize()
        assert float(out) == 0.0 and bool((n_img == -7.0).all()), (batch, h, w, T)
        assert not bool(ga_t.any()) and not bool(gp_t[:batch].any()), (batch, h, w, T)
    out = torch.full((1,), 5.0, device="cuda")
    _capi.check(lib.tsamd_normal_mse(None, 0, 0, None, 0, 0, 0, None, None, None, None, None, out.data_ptr(), None, None))
    torch.cuda.synchronize()
    assert float(out) == 0.0
    # ids that name no triangle of the list behave as background, bit for bit
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
    loss_f, n_f = dev.forward(attr, target, mask, ids=f_ids)
    loss_b, n_b = dev.forward(attr, target, mask, ids=b_ids)
    assert _bits(loss_f) == _bits(loss_b) and np.array_equal(n_f, n_b)
    assert np.all(n_f.reshape(-1, 3)[pick.cpu().numpy()] == 0.0)
    assert _bits(loss_f) != _bits(dev.forward(attr, target, mask)[0])
    ga_f, gp_f = dev.backward(attr, target, mask, ids=f_ids)
    ga_b, gp_b = dev.backward(attr, target, mask, ids=b_ids)
    _check_gradients("foreign ids", ga_f, gp_f, ga_b.astype(np.float64), gp_b.astype(np.float64))


def _chain(pos, tri, normals, res, target_alpha, target_normal, normal_mask, weights, depth=None):
    """The operator chain at the dr level: the detached losses (alpha[, depth], normal) and n, with their weighted sum backpropagated.
    ``depth``: (world, campos, target_depth, depth_mask)."""
    import torch
    import tssplat_amd.dr as dr
    ctx = dr.RasterizeCudaContext()
    mse = torch.nn.MSELoss()
    rast, _ = dr.rasterize(ctx, pos, tri, resolution=list(res), grad_db=False)
    alpha = torch.clamp(rast[..., -1:].detach(), 0, 1).contiguous()
    alpha = dr.antialias(alpha, rast, pos, tri, topology_hash=None, pos_gradient_boost=1.0)
    losses = [mse(alpha[..., -1], target_alpha)]
    if depth is not None:
        world, campos, target_depth, depth_mask = depth
        x, _ = dr.interpolate(world[None, ...], rast, tri)
        d = torch.norm(x - campos[:, None, None, :], dim=-1, keepdim=True)
        losses.append(mse(d[..., -1] * depth_mask, target_depth * depth_mask))
    n, _ = dr.interpolate(normals[None, ...], rast, tri)
    losses.append(mse(n * normal_mask[..., None], target_normal * normal_mask[..., None]))
    sum(w * k for w, k in zip(weights, losses)).backward()
    return [k.detach() for k in losses], n.detach()


@pytest.mark.gpu
@pytest.mark.parametrize("with_depth", [False, True], ids=["alpha_normal", "alpha_depth_normal"])
def test_silhouette_normal_mse_against_the_operators(with_depth):
    """dr.silhouette_normal_mse on the 33 x 50 scene against rasterize -> clamp -> antialias -> MSELoss plus interpolate -> masked
    MSELoss (and interpolate -> norm -> masked MSELoss with ``depth``): alpha_loss has dr.silhouette_mse's bits, depth_loss
    dr.silhouette_depth_mse's, normal_loss is within the loss bound of the chain's own n evaluated in float64, the gradients of a
    weighted sum within 2e-5 of their largest entries; one autograd node; both forms of normals and of the mask give equal bits."""
    import torch
    import tssplat_amd.dr as dr
    build, res = SCENES["checker_sheet"]
    pos_np, tri_np = build()
    B, V = pos_np.shape[:2]
    attr_np, target_np, mask_np = _inputs(B, V, res, seed=23)
    _assert_mixed(R.rasterize(pos_np, tri_np, res)[..., 3] > 0, mask_np)
    world_np, campos_np, depth_np, dmask_np = TD._inputs(B, V, res, seed=23)
    tri = torch.from_numpy(tri_np).cuda()
    target_normal, mask, campos, target_depth, depth_mask = (torch.from_numpy(k).cuda() for k in (target_np, mask_np, campos_np, depth_np, dmask_np))
    torch.manual_seed(5)
    target_alpha = torch.rand(B, *res, device="cuda")
    weights = (2000.0, 700.0, 900.0) if with_depth else (2000.0, 900.0)

    def leaves():
        return [torch.from_numpy(k).cuda().requires_grad_(True) for k in (pos_np, attr_np, world_np)]
    pos_c, normals_c, world_c = leaves()
    losses_c, n_chain = _chain(pos_c, tri, normals_c, res, target_alpha, target_normal, mask, weights,
                               depth=(world_c, campos, target_depth, depth_mask) if with_depth else None)
    pos, normals, world = leaves()
    ctx = dr.RasterizeCudaContext()
    depth = (world, campos, target_depth[..., None], depth_mask) if with_depth else None
    got = dr.silhouette_normal_mse(ctx, pos, tri, list(res), target_alpha, normals, target_normal, mask, depth=depth, return_images=True)
    k = 3 if with_depth else 2
    assert len(got) == 2 * k
    losses, images = got[:k], got[k:]
    assert all(t.dim() == 0 and t.grad_fn is losses[0].grad_fn for t in losses) and not any(t.requires_grad for t in images)
    assert [tuple(t.shape) for t in images] == [(B,) + res + (c,) for c in ((1, 1, 3) if with_depth else (1, 3))]
    other = (world[None], campos, target_depth, depth_mask[..., None]) if with_depth else None
    again = dr.silhouette_normal_mse(ctx, pos, tri, list(res), target_alpha[..., None], normals[None], target_normal, mask[..., None], depth=other)
    assert len(again) == k and [_bits(t.detach()) for t in again] == [_bits(t.detach()) for t in losses]
    assert _bits(dr.silhouette_mse(ctx, pos.detach(), tri, list(res), target_alpha)) == _bits(losses[0].detach())
    if with_depth:
        pair = dr.silhouette_depth_mse(ctx, pos.detach(), tri, list(res), target_alpha, world.detach(), campos, target_depth, depth_mask)
        assert _bits(pair[1]) == _bits(losses[1].detach())
    want, bound = N.loss_bound(n_chain.cpu().numpy(), target_np, mask_np)
    value = float(losses[-1].detach())
    print(f"dr: normal_loss {value:.9g} against the chain in float64 {want:.12g}, error / bound {abs(value - want) / bound:.3f}; "
          f"n against the chain's {float((images[-1] - n_chain).abs().max()):.3e}")
    assert want > 0 and abs(value - want) <= bound
    sum(w * t for w, t in zip(weights, losses)).backward()
    pairs = [("pos.grad", pos.grad, pos_c.grad), ("normals.grad", normals.grad, normals_c.grad)]
    if with_depth:
        pairs.append(("world_pos.grad", world.grad, world_c.grad))
    else:
        assert world.grad is None
    for label, got_g, want_g in pairs:
        scale = float(want_g.abs().max())
        err = float((got_g - want_g).abs().max())
        print(f"dr: {label} max {scale:.3e}, error {err:.3e} ({err / scale / GRAD_TOL:.3f} of the bound)")
        assert scale > 0 and err <= GRAD_TOL * scale
    with pytest.raises(RuntimeError, match="silhouette_normal_mse: normals must be"):
        dr.silhouette_normal_mse(ctx, pos, tri, list(res), target_alpha, normals[:-1], target_normal, mask, depth=depth)
    with pytest.raises(RuntimeError, match="silhouette_normal_mse: target_normal must be"):
        dr.silhouette_normal_mse(ctx, pos, tri, list(res), target_alpha, normals, target_normal[..., :2], mask, depth=depth)
    with pytest.raises(RuntimeError, match="silhouette_normal_mse: normal_mask must be"):
        dr.silhouette_normal_mse(ctx, pos, tri, list(res), target_alpha, normals, target_normal, mask[:, :-1], depth=depth)
    if with_depth:
        with pytest.raises(RuntimeError, match="silhouette_normal_mse: world_pos must be"):
            dr.silhouette_normal_mse(ctx, pos, tri, list(res), target_alpha, normals, target_normal, mask, depth=(world[:-1],) + depth[1:])
        with pytest.raises(RuntimeError, match="silhouette_normal_mse: campos must be"):
            dr.silhouette_normal_mse(ctx, pos, tri, list(res), target_alpha, normals, target_normal, mask, depth=(world, campos[:-1]) + depth[2:])
        with pytest.raises(RuntimeError, match="silhouette_normal_mse: depth must be"):
            dr.silhouette_normal_mse(ctx, pos, tri, list(res), target_alpha, normals, target_normal, mask, depth=depth[:3])


@pytest.mark.gpu
@pytest.mark.parametrize("with_depth", [False, True], ids=["alpha_normal", "alpha_depth_normal"])
def test_renderer_silhouette_normal_loss(aveg, with_depth):
    """MeshRasterizer.silhouette_normal_loss on the golden mesh, 2 views x 64^2, against the default forward(only_alpha=True,
    fit_normal=True[, fit_depth=True]) and the MSELoss calls: the losses within their bounds (the alpha loss: 4 * 2^-24 L, as
    tests/test_silhouette.py derives it), ``n`` within the per-component bound of its float64 evaluation and of out["n"],
    ``tet_v.grad`` of (20 img + 100 normal [+ 100 depth]) 100 + reg within 2e-5 of its largest entry; normal_mask=None is
    normal_mask=target_alpha."""
    import types
    import torch
    import tssplat_amd.dr as dr
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
    target_normal = torch.rand(2, 64, 64, 3, device="cuda", generator=gen) * 2 - 1
    mse = torch.nn.MSELoss()
    depth_kw = {"campos": campos, "target_depth": target_depth} if with_depth else {}

    geo.tet_v.grad = None
    out = ren(mvp, only_alpha=True, iter_num=5, resolution=64, fit_normal=True, fit_depth=with_depth, campos=campos if with_depth else None)
    img = mse(out["shaded"][..., -1], target_alpha) * 20
    img = img + mse(out["n"] * target_alpha[..., None], target_normal * target_alpha[..., None]) * 100
    if with_depth:
        img = img + mse(out["d"][..., -1] * target_alpha, target_depth * target_alpha) * 100
    (img * 100 + out["geo_regularization"]).backward()
    want_grad = geo.tet_v.grad.clone()
    frac = float((out["shaded"] > 0.5).float().mean())
    assert 0.05 < frac < 0.95

    geo.tet_v.grad = None
    got = ren.silhouette_normal_loss(mvp, target_alpha, target_normal, iter_num=5, resolution=64, **depth_kw)
    assert set(got) == {"img_loss", "normal_loss", "geo_regularization", "shaded", "n"} | ({"depth_loss", "d"} if with_depth else set())
    assert got["img_loss"].dim() == 0 and got["normal_loss"].dim() == 0 and not got["shaded"].requires_grad and not got["n"].requires_grad
    total = got["img_loss"] * 20 + got["normal_loss"] * 100
    if with_depth:
        assert got["depth_loss"].dim() == 0 and not got["d"].requires_grad
        total = total + got["depth_loss"] * 100
    (total * 100 + got["geo_regularization"]).backward()
    got_grad = geo.tet_v.grad.clone()

    alpha_np = target_alpha.cpu().numpy()
    want_img = float(mse(out["shaded"][..., -1].detach().double(), target_alpha.double()))
    img_loss = float(got["img_loss"].detach())
    want_normal, normal_bound = N.loss_bound(out["n"].detach().cpu().numpy(), target_normal.cpu().numpy(), alpha_np)
    normal_loss = float(got["normal_loss"].detach())
    print(f"renderer: img_loss error / bound {abs(img_loss - want_img) / (4 * D.U * want_img):.3f}, normal_loss {normal_loss:.9g} against "
          f"{want_normal:.12g}, error / bound {abs(normal_loss - want_normal) / normal_bound:.3f}")
    assert abs(img_loss - want_img) <= 4 * D.U * want_img
    assert want_normal > 0 and abs(normal_loss - want_normal) <= normal_bound
    if with_depth:
        want_depth, depth_bound = D.loss_bound(out["d"].detach().cpu().numpy()[..., 0], target_depth.cpu().numpy(), alpha_np)
        depth_loss = float(got["depth_loss"].detach())
        print(f"renderer: depth_loss {depth_loss:.9g} against {want_depth:.12g}, error / bound {abs(depth_loss - want_depth) / depth_bound:.3f}")
        assert want_depth > 0 and abs(depth_loss - want_depth) <= depth_bound
    assert float((got["shaded"] - out["shaded"].detach()).abs().max()) <= 2e-6
    # n against its own float64 evaluation, and against out["n"] (another float32 evaluation of the same expression)
    with torch.no_grad():
        data = geo(iter_num=5)
        pos_clip = ren.transform_pos(mvp, data.v_pos).contiguous()
        rast, _ = dr.rasterize(ren.glctx, pos_clip, data.t_pos_idx, resolution=[64, 64], grad_db=False)
        v_s = data._compute_vertex_normal() * torch.tensor([1, 1, -1], dtype=torch.float32, device="cuda")[None, :]
    n64, n_bound = N.normal_bound(rast.cpu().numpy(), data.t_pos_idx.cpu().numpy(), v_s.cpu().numpy())
    n_got = got["n"].cpu().numpy().astype(np.float64)
    n_chain = out["n"].detach().cpu().numpy().astype(np.float64)
    assert n_got.shape == (2, 64, 64, 3) and np.abs(n_got).max() > 0.5
    inside = n_bound > 0
    print(f"renderer: n error / bound {np.max(np.abs(n_got - n64)[inside] / n_bound[inside]):.3f} (against float64) "
          f"{np.max(np.abs(n_got - n_chain)[inside] / n_bound[inside]):.3f} (against out['n'])")
    assert np.all(np.abs(n_got - n64) <= n_bound) and np.all(np.abs(n_got - n_chain) <= n_bound)
    scale = float(want_grad.abs().max())
    err = float((got_grad - want_grad).abs().max())
    print(f"renderer: tet_v.grad max {scale:.3e}, fused against the chain {err:.3e} ({err / scale / GRAD_TOL:.3f} of the bound)")
    assert scale > 0 and err <= GRAD_TOL * scale
    same = ren.silhouette_normal_loss(mvp, target_alpha, target_normal, iter_num=5, resolution=64, normal_mask=target_alpha, **depth_kw)
    for name in ("normal_loss", "img_loss") + (("depth_loss",) if with_depth else ()):
        assert _bits(same[name].detach()) == _bits(got[name].detach()), name
    assert torch.equal(same["n"], got["n"])
