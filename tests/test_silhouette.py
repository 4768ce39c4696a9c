"""The alpha stage without a rast image: dr.silhouette / dr.silhouette_mse, the five tsamd_silhouette* entry points and the
opt-in callers in MeshRasterizer, against the operators path (rasterize -> clamp -> antialias [-> MSELoss]) and the float64 oracle
(tests/silhouette_oracle.py over oracle/raster_oracle.py).

CPU tier: the property the kernels rely on -- with colours in {0, 1} only pairs with exactly one background pixel change the
image or the gradient -- asserted on the oracle alone, and the argument checks of the C ABI.  GPU tier: every case asserts on the
GPU's own ``rast`` what its scene is there for before it looks at a kernel's output.
"""
import ctypes
import os

import numpy as np
import pytest

import aa_scenes as S
import silhouette_oracle as O
from oracle import raster_oracle as R

EPS = 2.0 ** -24     # unit round-off of float32


def masked_group(n_chunks):
    """Chunks per wave of the masked kernels (``masked_launch`` in aa_kernels.hip, restated: a property of the launch)."""
    g = 1
    while g < 64 and n_chunks // (2 * g) >= 16384:
        g *= 2
    return g


def _blends_per_pixel(events):
    count = {}
    for ev in events:
        count[ev[0]] = count.get(ev[0], 0) + 1
    return max(count.values(), default=0)


def _ragged(res, views):
    H, W = res
    if (H, W) == (33, 50):
        return S.merge(O.sparse_checker(H, W, 27, 3, 6, 47, views=views), S.open_sheet(H, W, views=views, box=(2, -1, 48, 25)))
    return S.merge(O.sparse_checker(H, W, 0, 1, 3, 191, views=views), S.open_sheet(H, W, nu=30, nv=5, views=views, box=(1, 3.5, 191, 7.5)))


def _backdrop_sheet(H, W):
    return S.merge(S.backdrop(H, W), S.open_sheet(H, W, nu=9, nv=8, views=1))


# ================================================================ CPU tier ================================================================

CPU_SCENES = {
    # name: (builder, resolution, least coverage events per view, foreground / foreground events expected)
    "sparse_checker": (lambda: O.sparse_checker(24, 160, 9, 10, 6, 140, views=2), (24, 160), 800, False),
    "checker_and_sheet": (lambda: _ragged((33, 50), 3), (33, 50), 200, True),
    "soup": (lambda: S.soup(48, 64), (48, 64), 25, True),
    "backdrop_and_sheet": (lambda: _backdrop_sheet(32, 32), (32, 32), 0, True),
}


@pytest.mark.parametrize("scene", sorted(CPU_SCENES))
def test_only_coverage_pairs_change_the_alpha_image(scene):
    """Events filtered to coverage pairs reproduce the unfiltered oracle exactly -- image and grad_pos -- because a pair of two
    covered pixels blends w (1 - 1) = 0 and scatters g 0."""
    build, res, least, both_expected = CPU_SCENES[scene]
    pos, tri = build()
    rast = R.rasterize(pos, tri, res)
    opp = R.edge_partners(tri)
    ev_all, ev_cov = O.events(rast, pos, tri, opp)
    cov = O.coverage(rast)
    # the scene's condition first
    n_both = [len(O.split_events(ev_all[b], cov[b])[1]) for b in range(len(ev_all))]
    if scene == "backdrop_and_sheet":
        assert cov.all() and not O.coverage_pairs(rast).any() and all(len(e) == 0 for e in ev_cov)
    else:
        assert min(len(e) for e in ev_cov) >= max(least, 1), [len(e) for e in ev_cov]
    assert (min(n_both) >= 20) if both_expected else (max(n_both) == 0), n_both
    if scene == "sparse_checker":
        per_chunk = O.coverage_pairs(rast).reshape(-1, 2).sum(axis=1)
        per_chunk = per_chunk[:len(per_chunk) // 64 * 64].reshape(-1, 64).sum(axis=1)
        assert (per_chunk == 128).sum() >= 8
    assert max(_blends_per_pixel(e) for e in ev_all) <= 4
    # every coverage event lies on a pair the coverage masks name
    pairs = O.coverage_pairs(rast)
    for b, evs in enumerate(ev_cov):
        for dst, src, _, _, axis, _, _ in evs:
            assert pairs[b, min(dst[0], src[0]), min(dst[1], src[1]), axis]
    g = np.random.default_rng(5).standard_normal(rast.shape[:3] + (1,))
    full = O.silhouette(rast, pos, tri, opp, events=ev_all)
    only = O.silhouette(rast, pos, tri, opp, events=ev_cov)
    assert np.array_equal(full, only)
    gp_full = O.silhouette_backward(rast, pos, tri, g, opp, 2.0, events=ev_all)
    gp_only = O.silhouette_backward(rast, pos, tri, g, opp, 2.0, events=ev_cov)
    assert np.array_equal(gp_full, gp_only)
    if scene == "backdrop_and_sheet":
        assert np.array_equal(full, np.ones_like(full)) and not gp_full.any()
    else:
        assert np.abs(gp_full).max() > 0 and (np.abs(full - O.clamp_image(rast)) > 0).sum() >= least // 2


def test_silhouette_abi_rejects_bad_arguments():
    """The five entry points check their arguments before any device call (this test runs without a GPU), with the limits and
    the messages of tsamd_rasterize; tsamd_silhouette_mse_workspace_bytes is monotone and 256-byte aligned."""
    from tssplat_amd import _capi
    lib = _capi.load()
    p = ctypes.c_void_p(256)                                       # a non-null pointer that is never dereferenced: every call below fails first

    def err(rc):
        assert rc != 0
        return lib.tsamd_last_error().decode()

    def fwd(batch=1, V=3, T=1, H=8, W=8, pos=p, tri=p, opp=p, ws=p, ids=p, masks=p, alpha=p):
        return lib.tsamd_silhouette(pos, batch, V, tri, T, opp, H, W, ws, ids, masks, alpha, None)

    def bwd(batch=1, V=3, T=1, H=8, W=8, pos=p, tri=p, opp=p, ids=p, masks=p, g=p, gp=p):
        return lib.tsamd_silhouette_backward(pos, batch, V, tri, T, opp, H, W, ids, masks, g, 1.0, gp, None)

    def mse_bwd(batch=1, V=3, T=1, H=8, W=8, pos=p, tri=p, opp=p, ids=p, masks=p, alpha=p, target=p, gl=p, gp=p):
        return lib.tsamd_silhouette_mse_backward(pos, batch, V, tri, T, opp, H, W, ids, masks, alpha, target, gl, 1.0, gp, None)

    for call in (fwd, bwd, mse_bwd):
        for kw in ({"H": 8193}, {"W": 8193}, {"batch": -1}, {"H": -1}):
            assert "out of range (0 .. 8192 pixels per side)" in err(call(**kw)), (call.__name__, kw)
        for kw in ({"T": 1 << 24}, {"T": -1}, {"V": -1}):
            assert "2^24 - 1 triangles" in err(call(**kw)), (call.__name__, kw)
        assert "grid limit" in err(call(batch=1 << 20, T=(1 << 24) - 1, H=0))
        for name in ("pos", "tri", "opp"):
            assert err(call(**{name: None})).endswith({"pos": "pos_clip_dev", "tri": "tri_dev", "opp": "edge_partner_dev"}[name] + " is null")
    for name, word in (("ws", "workspace_dev"), ("ids", "ids_out_dev"), ("masks", "cover_masks_out_dev"), ("alpha", "alpha_out_dev")):
        assert err(fwd(**{name: None})).endswith(word + " is null")         # (every pointer is named on its own)
    for call, names in ((bwd, (("ids", "ids_dev"), ("masks", "cover_masks_dev"), ("g", "grad_alpha_dev"), ("gp", "grad_pos_dev"))),
                        (mse_bwd, (("ids", "ids_dev"), ("masks", "cover_masks_dev"), ("alpha", "alpha_dev"), ("target", "target_dev"),
                                   ("gl", "grad_loss_dev"), ("gp", "grad_pos_dev")))):
        for name, word in names:
            assert err(call(**{name: None})).endswith(word + " is null"), (call.__name__, name)
    assert "negative size" in err(lib.tsamd_silhouette_mse(p, p, -1, p, p, None))
    assert "loss_out_dev is null" in err(lib.tsamd_silhouette_mse(p, p, 16, p, None, None))
    for k, word in ((0, "alpha_dev"), (1, "target_dev"), (3, "workspace_dev")):
        args = [p, p, 16, p, p, None]
        args[k] = None
        assert err(lib.tsamd_silhouette_mse(*args)).endswith(word + " is null")
    assert lib.tsamd_silhouette_mse_workspace_bytes(-1) == -1
    sizes = [0, 1, 3, 4, 1023, 1024, 1025, 4950, 1 << 20, (1 << 20) + 1, 120 * 512 * 512, 1 << 33]
    got = [lib.tsamd_silhouette_mse_workspace_bytes(n) for n in sizes]
    assert all(b > 0 and b % 256 == 0 for b in got) and got == sorted(got) and got[-1] > got[0]


# ================================================================ GPU tier ================================================================

def _operators_path(pos_np, tri_np, res, g_np, boost):
    """(rast, alpha, grad_pos) of rasterize -> clamp -> antialias on the device, as numpy."""
    import torch
    import tssplat_amd.dr as dr
    tri = torch.from_numpy(tri_np).cuda()
    pos = torch.from_numpy(pos_np).cuda().requires_grad_(True)
    rast, _ = dr.rasterize(dr.RasterizeCudaContext(), pos, tri, resolution=list(res), grad_db=False)
    alpha = torch.clamp(rast[..., -1:].detach(), 0, 1).contiguous()
    out = dr.antialias(alpha, rast, pos, tri, topology_hash=None, pos_gradient_boost=boost)
    out.backward(torch.from_numpy(g_np).cuda())
    return rast.detach().cpu().numpy(), out.detach().cpu().numpy(), pos.grad.cpu().numpy()


def _grad_bound(count, mass):
    """Per entry ``2^-24 (n + 3) M + 1e-30`` -- n fp32 atomic additions, one rounding of every term, a one-term fp32 product (the
    ``dense`` bound of tests/test_antialias_edges.py::check_antialias with one channel) -- and exactly zero where n = 0."""
    return np.where(count[..., None] > 0, EPS * (count[..., None] + 3) * mass + 1e-30, 0.0)


def check_silhouette(pos_np, tri_np, res, condition, min_changed, boost=2.0, seed=7):
    """The one comparison every forward / backward case goes through; returns what the MSE tests reuse."""
    import torch
    import tssplat_amd.dr as dr
    B, V = pos_np.shape[:2]
    H, W = res
    g_np = np.random.default_rng(seed).standard_normal((B, H, W, 1), dtype=np.float32)
    rast, op_alpha, op_gp = _operators_path(pos_np, tri_np, res, g_np, boost)
    tri = torch.from_numpy(tri_np).cuda()
    pos = torch.from_numpy(pos_np).cuda().requires_grad_(True)
    alpha_d = dr.silhouette(dr.RasterizeCudaContext(), pos, tri, list(res), topology_hash=None, pos_gradient_boost=boost)
    assert alpha_d.shape == (B, H, W, 1) and alpha_d.dtype == torch.float32
    alpha_d.backward(torch.from_numpy(g_np).cuda())
    alpha, gp = alpha_d.detach().cpu().numpy(), pos.grad.cpu().numpy()

    opp = R.edge_partners(tri_np)
    ref = np.empty((B, H, W, 1))
    ref_gp = np.empty((B, V, 4))
    ev_all, ev_cov = [], []
    for b in range(B):                                             # one view at a time: the large cases stay flat in host memory
        sl = slice(b, b + 1)
        ea, ec = O.events(rast[sl], pos_np[sl], tri_np, opp)
        ev_all.append(ea[0])
        ev_cov.append(ec[0])
        ref[sl] = O.silhouette(rast[sl], pos_np[sl], tri_np, opp, events=ea)
        ref_gp[sl] = O.silhouette_backward(rast[sl], pos_np[sl], tri_np, g_np[sl], opp, boost, events=ea)
    condition(rast, ev_all, ev_cov)
    assert max(_blends_per_pixel(e) for e in ev_all) <= 4
    cov01 = O.clamp_image(rast)
    untouched = np.ones((B, H, W), dtype=bool)
    for b in range(B):
        for ev in ev_cov[b]:
            untouched[b][ev[0]] = False
    n_changed = int((np.abs(ref - cov01) > 0).sum())
    count, mass = O.gradient_terms(ev_cov, pos_np, g_np, res, boost)
    tol = _grad_bound(count, mass)
    print(f"silhouette case {B}x{H}x{W}: {sum(len(e) for e in ev_cov)} coverage events of {sum(len(e) for e in ev_all)} on {n_changed} pixels, "
          f"{int(O.coverage_pairs(rast).sum())} coverage pairs; alpha error {np.abs(alpha - ref).max():.3e} (oracle) {np.abs(alpha - op_alpha).max():.3e} "
          f"(operators); grad_pos error / bound {np.max(np.abs(gp - ref_gp) / np.maximum(tol, 1e-300)):.3f} (fused) "
          f"{np.max(np.abs(op_gp - ref_gp) / np.maximum(tol, 1e-300)):.3f} (operators)")
    assert n_changed >= min_changed
    assert np.all(np.abs(alpha - ref) <= 2e-6) and np.all(np.abs(alpha - op_alpha) <= 2e-6)
    assert np.array_equal(alpha[untouched], cov01[untouched])
    assert np.all(np.abs(gp - ref_gp) <= tol)
    assert np.all(gp[count == 0] == 0.0)
    assert np.all(np.abs(gp - op_gp) <= 2 * tol)                  # (the operators path is within the same bound of the oracle)
    if min_changed:
        assert np.abs(ref_gp).max() > 0
    return rast, alpha, ev_all, ev_cov, opp


def _ragged_condition(views, res):
    H, W = res

    def condition(rast, ev_all, ev_cov):
        flat = O.coverage_pairs(rast).reshape(-1, 2).any(axis=1)
        for unit in [u for u in (64,) if (H * W) % u != 0]:
            for b in range(1, views):                              # the chunk that straddles views b - 1 | b: pairs on both sides
                k = b * H * W // unit
                assert flat[unit * k:b * H * W].any() and flat[b * H * W:unit * (k + 1)].any()
        if (views * H * W) % 64 != 0:
            assert flat[len(flat) // 64 * 64:].any()               # the partial chunk at the end
        cov = O.coverage(rast)
        # without the guards the last column would pair with the next row's first pixel, the last row with the next view's first
        assert (cov[:, :-1, -1] != cov[:, 1:, 0]).any() and (cov[:-1, -1, :] != cov[1:, 0, :]).any()
        pairs = O.coverage_pairs(rast)
        assert pairs[:, -1, :, 0].any() and pairs[:, :, -1, 1].any()      # pairs inside the last row and inside the last column
        assert all(len(e) > 100 for e in ev_cov)
        assert all(len(a) > len(c) for a, c in zip(ev_all, ev_cov))     # the sheet's folds: foreground / foreground events, filtered out
    return condition


@pytest.mark.gpu
@pytest.mark.parametrize("views,res", [(3, (33, 50)), (2, (7, 192))])
def test_silhouette_on_views_that_end_inside_a_chunk(views, res):
    """Views that end inside a 64-pixel chunk (33 x 50), a partial last chunk, coverage pairs in the last row and column."""
    pos, tri = _ragged(res, views)
    assert ((views * res[0] * res[1]) % 64 != 0) == (res == (33, 50))
    check_silhouette(pos, tri, res, _ragged_condition(views, res), 200)


def _full_chunks_condition(rast, ev_all, ev_cov):
    per_chunk = O.coverage_pairs(rast).reshape(-1, 64, 2).sum(axis=(1, 2))
    assert (per_chunk == 128).sum() >= 8
    assert all(len(a) == len(c) and len(c) > 800 for a, c in zip(ev_all, ev_cov))


@pytest.mark.gpu
def test_silhouette_on_full_chunks():
    """Every pixel of the band carries a coverage pair on both axes: chunks with all 128 mask bits set."""
    H, W = 24, 160
    pos, tri = O.sparse_checker(H, W, 9, 10, 6, 140, views=2)
    check_silhouette(pos, tri, (H, W), _full_chunks_condition, 800)


def _open_mesh_condition(scene, pos, tri):
    def condition(rast, ev_all, ev_cov):
        slots = S.edge_slots(tri)
        for b in range(2):
            n_boundary = sum(len(slots[(min(ev[5]), max(ev[5]))]) == 1 for ev in ev_cov[b])
            assert n_boundary >= (100 if scene == "open_sheet" else 20)
            assert len(ev_all[b]) - len(ev_cov[b]) >= 20                # foreground / foreground events exist and are filtered out
            if scene == "soup":
                # covered pixels that show a triangle with a vertex that cannot be projected (clipped at the near plane), and
                # coverage pairs at them: analysed, blend nothing
                ids = rast[b, ..., 3].astype(np.int64) - 1
                bad_tri = (~S.projectable(pos[b])[tri]).any(axis=1)
                covered_bad = (ids >= 0) & bad_tri[np.maximum(ids, 0)]
                pairs = O.coverage_pairs(rast)[b]
                at_bad = (pairs[:, :-1, 0] & (covered_bad[:, :-1] | covered_bad[:, 1:])).sum() + (pairs[:-1, :, 1] & (covered_bad[:-1] | covered_bad[1:])).sum()
                assert covered_bad.sum() >= 50 and at_bad >= 3
        if scene == "soup":
            assert sum(len(slots[(min(ev[5]), max(ev[5]))]) >= 3 for b in range(2) for ev in ev_all[b]) >= 3      # three-triangle edges
    return condition


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["open_sheet", "soup"])
def test_silhouette_on_open_and_non_manifold_meshes(scene):
    """Boundary edges, edges with three triangles, and triangles with a vertex at w <= 0 / NaN: covered (clipped at the near
    plane: alpha 1) but their silhouette is not blended."""
    H, W = 48, 64
    pos, tri = S.open_sheet(H, W, views=2) if scene == "open_sheet" else S.soup(H, W)
    check_silhouette(pos, tri, (H, W), _open_mesh_condition(scene, pos, tri), 150 if scene == "open_sheet" else 50)


@pytest.mark.gpu
def test_silhouette_of_a_fully_covered_view():
    """A backdrop behind an open sheet: no coverage pair anywhere, alpha all 1, gradient all 0."""
    import torch
    import tssplat_amd.dr as dr
    H, W = 32, 32
    pos, tri = _backdrop_sheet(H, W)

    def condition(rast, ev_all, ev_cov):
        assert O.coverage(rast).all() and len(ev_cov[0]) == 0 and len(ev_all[0]) >= 100

    _, alpha, _, _, _ = check_silhouette(pos, tri, (H, W), condition, 0)
    assert np.array_equal(alpha, np.ones_like(alpha))
    pos_d = torch.from_numpy(pos).cuda().requires_grad_(True)
    dr.silhouette(dr.RasterizeCudaContext(), pos_d, torch.from_numpy(tri).cuda(), [H, W]).sum().backward()
    assert float(pos_d.grad.abs().max()) == 0.0


@pytest.mark.gpu
def test_silhouette_with_waves_that_own_two_chunks():
    """2 x 1025 x 1025: ``masked_group`` 2, the last wave short of chunks and the last chunk of pixels, a dense band."""
    views, side = 2, 1025
    pos, tri = O.sparse_checker(side, side, 500, 300, 5, 330, views=views)
    n_chunks = (views * side * side + 63) // 64
    assert masked_group(n_chunks) == 2 and n_chunks % 2 != 0 and (views * side * side) % 64 != 0

    def condition(rast, ev_all, ev_cov):
        c = O.coverage_pairs(rast).reshape(-1, 2).sum(axis=1)
        per_chunk = np.concatenate([c, np.zeros(n_chunks * 64 - len(c), dtype=c.dtype)]).reshape(n_chunks, 64).sum(axis=1)
        runs, deepest = S.dense_aligned_runs(per_chunk, 2, at_least=100)
        assert runs >= 1 and deepest >= 200

    check_silhouette(pos, tri, (side, side), condition, 150 * 5 * views)


@pytest.mark.gpu
def test_silhouette_ids_and_cover_masks_through_the_c_abi():
    """tsamd_silhouette's by-products: ids equal rast's fourth channel, the coverage masks equal the ones numpy builds from it
    (chunks that straddle views, the partial last chunk, the last row and column)."""
    import torch
    import tssplat_amd.dr as dr
    from tssplat_amd import _capi
    lib = _capi.load()
    for views, res in ((3, (33, 50)), (2, (7, 192)), (2, (48, 64))):
        H, W = res
        pos_np, tri_np = _ragged(res, views) if res != (48, 64) else S.soup(H, W)
        pos, tri = torch.from_numpy(pos_np).cuda(), torch.from_numpy(tri_np).cuda()
        rast, _ = dr.rasterize(dr.RasterizeCudaContext(), pos, tri, resolution=[H, W], grad_db=False)
        topo = dr.antialias_construct_topology_hash(tri)
        B, V, T = views, pos.shape[1], tri.shape[0]
        ws = torch.empty(lib.tsamd_rasterize_workspace_bytes(B, V, H, W), dtype=torch.uint8, device="cuda")
        ids = torch.full((B, H, W), -7, dtype=torch.int32, device="cuda")
        n_mask = lib.tsamd_pair_masks_bytes(B, H, W)
        masks = torch.full((n_mask // 8 + 4,), -1, dtype=torch.int64, device="cuda")       # (4 guard words behind the masks)
        alpha = torch.full((B, H, W, 1), -7.0, device="cuda")
        _capi.check(lib.tsamd_silhouette(pos.data_ptr(), B, V, tri.data_ptr(), T, topo.opp.data_ptr(), H, W, ws.data_ptr(), ids.data_ptr(),
                                         masks.data_ptr(), alpha.data_ptr(), None))
        torch.cuda.synchronize()
        rast_np = rast.cpu().numpy()
        assert np.array_equal(ids.cpu().numpy(), rast_np[..., 3].astype(np.int32))
        got = masks.cpu().numpy().view(np.uint64)
        assert np.array_equal(got[:n_mask // 8].reshape(-1, 2), O.cover_masks(rast_np))
        assert np.all(got[n_mask // 8:] == np.uint64(0xFFFFFFFFFFFFFFFF))
        assert O.cover_masks(rast_np).any()


@pytest.mark.gpu
def test_silhouette_on_empty_inputs():
    """Batch 0, an image without pixels, no triangles: success, alpha all zero, zero gradients, loss 0 of nothing."""
    import torch
    import tssplat_amd.dr as dr
    from tssplat_amd import _capi
    ctx = dr.RasterizeCudaContext()
    no_tri = torch.zeros((0, 3), dtype=torch.int32, device="cuda")
    one_tri = torch.tensor([[0, 1, 2]], dtype=torch.int32, device="cuda")
    pos = torch.tensor([[[-0.5, -0.5, 0.0, 1.0], [0.5, -0.5, 0.0, 1.0], [0.0, 0.5, 0.0, 1.0]]], device="cuda")
    a = dr.silhouette(ctx, pos.clone().requires_grad_(True), no_tri, [16, 24])
    assert a.shape == (1, 16, 24, 1) and float(a.detach().abs().max()) == 0.0
    p = pos.clone().requires_grad_(True)
    target = torch.rand(1, 16, 24, device="cuda")
    loss = dr.silhouette_mse(ctx, p, no_tri, [16, 24], target)
    assert abs(float(loss.detach()) - O.mse(np.zeros((1, 16, 24)), target.cpu().numpy())) <= 4 * EPS * float(loss.detach())
    loss.backward()
    assert float(p.grad.abs().max()) == 0.0
    assert dr.silhouette(ctx, pos[:0], one_tri, [16, 24]).shape == (0, 16, 24, 1)
    for res in ([0, 24], [16, 0]):
        p = pos.clone().requires_grad_(True)
        a = dr.silhouette(ctx, p, one_tri, res)
        assert a.shape == (1, res[0], res[1], 1)
        a.sum().backward()
        assert float(p.grad.abs().max()) == 0.0
        assert float(dr.silhouette_mse(ctx, pos, one_tri, res, torch.zeros(1, res[0], res[1], device="cuda"))) == 0.0
    lib = _capi.load()
    out = torch.full((1,), 5.0, device="cuda")
    _capi.check(lib.tsamd_silhouette_mse(None, None, 0, None, out.data_ptr(), None))
    assert float(out) == 0.0
    with pytest.raises(RuntimeError, match="target must be"):
        dr.silhouette_mse(ctx, pos, one_tri, [16, 24], torch.zeros(1, 16, 25, device="cuda"))
    with pytest.raises(RuntimeError, match="pos must be"):
        dr.silhouette(ctx, pos[0], one_tri, [16, 24])


def _mse_through_the_c_abi(alpha, target):
    import torch
    from tssplat_amd import _capi
    lib = _capi.load()
    n = alpha.numel()
    ws = torch.empty(lib.tsamd_silhouette_mse_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    out = torch.empty(1, device="cuda")
    _capi.check(lib.tsamd_silhouette_mse(alpha.data_ptr(), target.data_ptr(), n, ws.data_ptr(), out.data_ptr(), None))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["4950", "7680", "aligned_2M+3", "unaligned_2M+3"])
def test_silhouette_mse_value_and_repeatability(case):
    """|loss - loss64(alpha_gpu)| <= 4 * 2^-24 * loss64: one rounding of the difference (2 u on its square), the final float
    rounding, the double sums negligible.  Two calls on the same tensor give equal bits.  n = 4 950 is no multiple of 4; 2^21 + 3
    elements take several rounds of the grid-stride loop, once through 16-byte loads and once (a pointer off by one float) not."""
    import torch
    import tssplat_amd.dr as dr
    torch.manual_seed(3)
    if case in ("4950", "7680"):
        views, res = (3, (33, 50)) if case == "4950" else (2, (24, 160))
        pos_np, tri_np = _ragged(res, views) if case == "4950" else O.sparse_checker(24, 160, 9, 10, 6, 140, views=2)
        pos, tri = torch.from_numpy(pos_np).cuda(), torch.from_numpy(tri_np).cuda()
        target = torch.rand(views, *res, device="cuda")
        loss, alpha = dr.silhouette_mse(dr.RasterizeCudaContext(), pos, tri, list(res), target, return_alpha=True)
        assert loss.dim() == 0 and alpha.shape == (views,) + res + (1,) and alpha.numel() == int(case) and not alpha.requires_grad
        assert float(alpha.min()) >= 0.0 and float(alpha.max()) <= 1.0 and 0.02 < float(alpha.mean()) < 0.98
    else:
        n = (1 << 21) + 3
        off = 1 if case.startswith("unaligned") else 0
        alpha = torch.rand(n + 4, device="cuda")[off:off + n]
        target = torch.rand(n + 4, device="cuda")[off:off + n]
        assert (alpha.data_ptr() % 16 == 0) == (off == 0) and (target.data_ptr() % 16 == 0) == (off == 0)
        loss = _mse_through_the_c_abi(alpha, target)[0]
    want = O.mse(alpha.cpu().numpy(), target.cpu().numpy())
    print(f"mse {case}: {float(loss):.9g} against {want:.12g}, error / bound {abs(float(loss) - want) / (4 * EPS * want):.3f}")
    assert want > 0 and abs(float(loss) - want) <= 4 * EPS * want
    assert alpha.is_contiguous() and target.is_contiguous()
    first, second = _mse_through_the_c_abi(alpha, target), _mse_through_the_c_abi(alpha, target)
    assert first.view(torch.int32).item() == second.view(torch.int32).item() == loss.reshape(1).view(torch.int32).item()


@pytest.mark.gpu
@pytest.mark.parametrize("views,res", [(3, (33, 50)), (2, (48, 64))])
def test_silhouette_mse_backward(views, res):
    """Upstream gradient 2 000 and boost 2, against the oracle fed with the GPU's own alpha image: grad_out = 2 (alpha - target)
    2 000 / n, per entry within the bound of check_silhouette.  No gradient image exists on the device path."""
    import torch
    import tssplat_amd.dr as dr
    H, W = res
    pos_np, tri_np = _ragged(res, views) if res == (33, 50) else S.soup(H, W)
    tri = torch.from_numpy(tri_np).cuda()
    pos = torch.from_numpy(pos_np).cuda().requires_grad_(True)
    torch.manual_seed(5)
    target = torch.rand(views, H, W, 1, device="cuda")
    ctx = dr.RasterizeCudaContext()
    loss, alpha = dr.silhouette_mse(ctx, pos, tri, [H, W], target, pos_gradient_boost=2.0, return_alpha=True)
    (loss * 2000.0).backward()
    gp = pos.grad.cpu().numpy()
    rast, _ = dr.rasterize(ctx, pos.detach(), tri, resolution=[H, W], grad_db=False)
    rast = rast.cpu().numpy()
    opp = R.edge_partners(tri_np)
    ev_all, ev_cov = O.events(rast, pos_np, tri_np, opp)
    assert all(len(e) >= 25 for e in ev_cov)                      # (the soup's second view is covered almost everywhere)
    g = O.mse_grad(alpha.cpu().numpy(), target.cpu().numpy(), 2000.0)
    want = O.silhouette_backward(rast, pos_np, tri_np, g, opp, 2.0, events=ev_all)
    count, mass = O.gradient_terms(ev_cov, pos_np, g, res, 2.0)
    tol = _grad_bound(count, mass)
    print(f"mse backward {views}x{H}x{W}: |grad_pos| max {np.abs(want).max():.3e}, error / bound {np.max(np.abs(gp - want) / np.maximum(tol, 1e-300)):.3f}")
    assert np.abs(want).max() > 0
    assert np.all(np.abs(gp - want) <= tol) and np.all(gp[count == 0] == 0.0)


@pytest.mark.gpu
def test_renderer_fused_silhouette(aveg):
    """MeshRasterizer(fused_silhouette=True) on the golden mesh, 2 views x 64^2: ``shaded`` within 2e-6 of the default path,
    ``tet_v.grad`` of the image term within 2e-5 of its largest entry (the bound tests/test_raster.py holds the antialias term of
    ``pos.grad`` to: fp32 atomics in arbitrary order), ``fit_depth=True`` falls back to the operators path and returns ``"d"``,
    and ``silhouette_loss`` is the mean squared error of the default path's ``shaded``.

    The loss bound is the kernel's own 4 * 2^-24 * L against MSELoss evaluated in float64 (the reference adds no rounding of its
    own); the two paths' images differ, if at all, in the last bit of a pixel that receives two blends, which moves the mean by
    ~1e-10 L."""
    import types
    import torch
    from tssplat_amd import geometry, renderers
    flags = types.SimpleNamespace(smooth_eng_coeff=2e-4, barrier_coeff=2e-4, increase_order_iter=1000)
    rest, tets = aveg
    geo = geometry.TetMeshGeometry(rest, tets, smooth_barrier_param=flags)
    default, fused = renderers.MeshRasterizer(geo), renderers.MeshRasterizer(geo, fused_silhouette=True)
    assert default.fused_silhouette is False
    mvp = torch.from_numpy(R.orbit_mvps(2)).cuda()
    campos = torch.tensor([[0.0, 1.0, 3.0]] * 2, device="cuda")
    g = torch.randn(2, 64, 64, 1, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    grads, shaded = {}, {}
    for name, ren in (("default", default), ("fused", fused)):
        geo.tet_v.grad = None
        out = ren(mvp, only_alpha=True, iter_num=5, resolution=64)
        assert set(out) == {"shaded", "geo_regularization"} and out["shaded"].shape == (2, 64, 64, 1)
        out["shaded"].backward(g)
        grads[name], shaded[name] = geo.tet_v.grad.clone(), out["shaded"].detach()
    frac = float((shaded["default"] > 0.5).float().mean())
    assert 0.05 < frac < 0.95 and float(((shaded["default"] > 0) & (shaded["default"] < 1)).sum()) >= 20
    assert float((shaded["fused"] - shaded["default"]).abs().max()) <= 2e-6
    scale = float(grads["default"].abs().max())
    err = float((grads["fused"] - grads["default"]).abs().max())
    print(f"renderer: tet_v.grad max {scale:.3e}, fused against default {err:.3e} ({err / scale:.2e} of the largest entry)")
    assert scale > 0 and err <= 2e-5 * scale
    with torch.no_grad():
        a = default(mvp, only_alpha=True, iter_num=5, resolution=64, fit_depth=True, campos=campos)
        b = fused(mvp, only_alpha=True, iter_num=5, resolution=64, fit_depth=True, campos=campos)
    assert "d" in b and torch.equal(a["d"], b["d"]) and float((a["shaded"] - b["shaded"]).abs().max()) <= 2e-6
    target = torch.rand(2, 64, 64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    geo.tet_v.grad = None
    got = fused.silhouette_loss(mvp, target, iter_num=5, resolution=64)
    assert set(got) == {"img_loss", "geo_regularization", "shaded"} and got["img_loss"].dim() == 0 and not got["shaded"].requires_grad
    want = float(torch.nn.MSELoss()(shaded["default"][..., -1].double(), target.double()))
    own = O.mse(got["shaded"].cpu().numpy(), target.cpu().numpy())
    img = float(got["img_loss"].detach())
    print(f"renderer: silhouette_loss {img:.9g}, MSELoss of the default path {want:.12g}, error / bound {abs(img - want) / (4 * EPS * want):.3f}")
    assert abs(img - own) <= 4 * EPS * own
    assert abs(img - want) <= 4 * EPS * want
    assert float((got["shaded"] - shaded["default"]).abs().max()) <= 2e-6
    (got["img_loss"] * 2000.0 + got["geo_regularization"]).backward()
    fused_grad = geo.tet_v.grad.clone()
    geo.tet_v.grad = None
    out = default(mvp, only_alpha=True, iter_num=5, resolution=64)
    (torch.nn.MSELoss()(out["shaded"][..., -1], target) * 2000.0 + out["geo_regularization"]).backward()
    scale = float(geo.tet_v.grad.abs().max())
    assert float((fused_grad - geo.tet_v.grad).abs().max()) <= 2e-5 * scale
