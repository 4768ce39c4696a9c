"""The rasteriser core (tssplat_amd/csrc/raster_kernels.hip: snap, bin, clip, resolve, silhouette_cover, rasterize_backward;
interpolate_kernels.hip: interpolate, interpolate_backward) pinned BIT FOR BIT and at every walk and launch edge.

Values: tests/raster_f32_oracle.py states the kernels' float32 operations in numpy; a CPU test ties it to the float64 oracle
(oracle/raster_oracle.py) within a derived rounding bound, the GPU tests compare the device with it by ``np.array_equal`` on
the raw bits.  Sums whose order varies (wave scan + fp32 atomics) are compared bit for bit on data that make every partial sum exact,
and on random data against the any-order summation bound ``gamma_(n-1) sum |c_i|`` -- nothing in it is chosen.

Edges: every fixture has a CPU test that shows FROM THE ORACLE (or the emulator of the pixel walk's fragment queue) that it reaches
its edge, and a GPU test that compares the depth keys (depth and id), ``rast``, the pair masks and the alpha stage's ids and coverage
masks bit for bit.  Power-of-two image sides with ``w = 1`` make snapped coordinates exact: ``x = X / (128 W) - 1`` lands on
sub-pixel ``X``, so vertices sit on chosen integers.
"""
import functools

import numpy as np
import pytest

import raster_f32_oracle as F
import silhouette_oracle as SO
from oracle import raster_oracle as R

U = F.U
NO = R.NO_FRAGMENT
LIMIT = R.COORD_LIMIT


# ------------------------------------------------------------ shared plumbing ------------------------------------------------------------

_key_cache = {}


def oracle_keys(pos, tri, res):
    """``rasterize_ids`` per view, computed once per distinct (view, triangle list, resolution) of the whole session."""
    H, W = res
    out = []
    th = hash(np.ascontiguousarray(tri).tobytes())
    for b in range(pos.shape[0]):
        k = (hash(np.ascontiguousarray(pos[b]).tobytes()), th, H, W)
        if k not in _key_cache:
            _key_cache[k] = R.rasterize_ids(pos[b], tri, H, W)
        out.append(_key_cache[k])
    return np.stack(out)


def oracle_rast(pos, tri, res):
    keys = oracle_keys(pos, tri, res)
    rast, zero_sign = F.resolve32(pos, tri, keys)
    return rast, zero_sign, keys


def pack_bits(bits):
    """``bits[n, 2]`` bool -> ``uint64[ceil(n / 64), 2]``: the layout of the pair masks and the coverage masks."""
    n = (len(bits) + 63) // 64
    full = np.zeros((n * 64, 2), dtype=bool)
    full[:len(bits)] = bits
    return (full.reshape(n, 64, 2).astype(np.uint64) << np.arange(64, dtype=np.uint64)[None, :, None]).sum(axis=1, dtype=np.uint64)


def pair_masks_of(ids):
    """Pair masks of an id image ``[B, H, W]``: the pixel's triangle differs from its right / upper neighbour's."""
    c = np.zeros(ids.shape + (2,), dtype=bool)
    c[:, :, :-1, 0] = ids[:, :, 1:] != ids[:, :, :-1]
    c[:, :-1, :, 1] = ids[:, 1:, :] != ids[:, :-1, :]
    return pack_bits(c.reshape(-1, 2))


def subpixel_vertices(points, res):
    """``[V, 4]`` float32 clip-space vertices with ``w = 1`` from ``(X, Y, z)`` in sub-pixel units: exact for power-of-two sides."""
    H, W = res
    p = np.array([[X / (128.0 * W) - 1.0, Y / (128.0 * H) - 1.0, z, 1.0] for X, Y, z in points])
    assert np.array_equal(p[:, :2].astype(np.float32).astype(np.float64), p[:, :2]), "coordinates are not exact in float32"
    return p.astype(np.float32)


def device_rasterize(pos, tri, res, want_masks=True):
    """``(keys, rast, pair masks)`` of tsamd_rasterize as numpy; the depth keys are the head of the workspace.  ``want_masks=False``:
    the call passes no mask buffer (the resolve pass then loads no neighbour key), and the buffer comes back untouched."""
    import torch
    from tssplat_amd import _capi
    lib = _capi.load()
    (B, V), T, (H, W) = pos.shape[:2], tri.shape[0], res
    pos_d, tri_d = torch.from_numpy(pos).cuda(), torch.from_numpy(np.ascontiguousarray(tri)).cuda()
    ws = torch.zeros(int(lib.tsamd_rasterize_workspace_bytes(B, V, H, W)), dtype=torch.uint8, device="cuda")
    rast = torch.full((B, H, W, 4), float("nan"), device="cuda")
    nm = int(lib.tsamd_pair_masks_bytes(B, H, W))
    assert nm == (B * H * W + 63) // 64 * 16
    masks = torch.full((nm,), 0xAB, dtype=torch.uint8, device="cuda")
    _capi.check(lib.tsamd_rasterize(pos_d.data_ptr(), B, V, tri_d.data_ptr(), T, H, W, ws.data_ptr(), rast.data_ptr(),
                                    masks.data_ptr() if want_masks else None, None))
    torch.cuda.synchronize()
    keys = ws[:B * H * W * 8].cpu().numpy().view(np.uint64).reshape(B, H, W)
    return keys, rast.cpu().numpy(), masks.cpu().numpy().view(np.uint64).reshape(-1, 2)


def device_silhouette(pos, tri, res):
    """``(alpha [B, H, W, 1], ids [B, H, W], coverage masks)`` of tsamd_silhouette (what ``dr.silhouette`` runs) as numpy."""
    import torch
    import tssplat_amd.dr as dr
    pos_d, tri_d = torch.from_numpy(pos).cuda(), torch.from_numpy(np.ascontiguousarray(tri)).cuda()
    topo = dr.antialias_construct_topology_hash(tri_d)
    alpha, ids, masks = dr._silhouette_forward(pos_d, tri_d, topo.opp, dr.RasterizeCudaContext(), res[0], res[1])
    n = (pos.shape[0] * res[0] * res[1] + 63) // 64 * 16
    return alpha.cpu().numpy(), ids.cpu().numpy(), masks[:n].cpu().numpy().view(np.uint64).reshape(-1, 2)


def check_device(pos, tri, res, full_alpha=False):
    """The one GPU comparison of every edge fixture: depth keys, ``rast``, pair masks, and the alpha stage's ids, coverage masks and
    alpha, against the oracles, bit for bit."""
    want, zero_sign, keys = oracle_rast(pos, tri, res)
    got_keys, got, masks = device_rasterize(pos, tri, res)
    assert np.array_equal(got_keys, keys), "depth keys (depth32 << 32 | triangle) differ"
    assert F.same_bits(got, want), f"{int(zero_sign.sum())} pixels with a -0 barycentric; rast differs in {int((got.view(np.uint32) != want.view(np.uint32)).any(-1).sum())} pixels"
    ids = F.ids_of(keys)
    assert np.array_equal(masks, pair_masks_of(ids))
    alpha, sil_ids, cover = device_silhouette(pos, tri, res)
    assert np.array_equal(sil_ids, (ids + 1).astype(np.int32))
    assert np.array_equal(cover, SO.cover_masks(want))
    pairs = SO.coverage_pairs(want)
    touched = pairs.any(-1)
    touched[:, :, 1:] |= pairs[:, :, :-1, 0]
    touched[:, 1:, :] |= pairs[:, :-1, :, 1]
    cov01 = (ids >= 0).astype(np.float32)
    assert np.array_equal(alpha[..., 0][~touched], cov01[~touched])          # no coverage pair: nothing is blended
    assert np.isfinite(alpha).all()
    if full_alpha:
        ref = SO.silhouette(want, pos, tri)
        assert np.abs(alpha - ref).max() <= 2e-6                             # (tests/test_silhouette.py's tolerance for the blends)
    return got


# ------------------------------------------------ A. the float32 statement against the float64 oracle ------------------------------------------------

def _kuhn4_scene():
    from tssplat_amd import geometry, scenes
    sc = scenes.make_scene("kuhn4", 3, seed=0)
    vid, faces = geometry.get_surface_vf(sc.tets)
    v = scenes.deform(sc, 0.05, seed=1)[np.asarray(vid)]
    return R.transform_pos(R.orbit_mvps(2), v), np.asarray(faces, dtype=np.int32), v


def _uv_bound(p, tri, keys):
    """First-order forward error bound of the float32 value path, from FLOAT64 values only.  With U = 2^-24 and |f| <= 1:

        f   = ((i + 0.5) / W) 2 - 1        i + 0.5 and the doubling are exact: one rounding of the quotient (doubled: <= U |f + 1| <= 2U)
                                           and one of the difference (U |f|)                                             df <= 3U
        p_k = x_k - f w_k                  |w_k| df + U |f w_k| (product) + U |p_k| (difference)                        dp_k <= 4U |w_k| + U |p_k|
        a_0 = p1x p2y - p1y p2x            dp1x |p2y| + |p1x| dp2y + dp1y |p2x| + |p1y| dp2x + U (|p1x p2y| + |p1y p2x|) + U |a_0|
        s   = (a_0 + a_1) + a_2            da_0 + da_1 + da_2 + 2U (|a_0| + |a_1| + |a_2|)
        b_k = a_k / s                      da_k / |s| + |a_k| ds / s^2 + U |b_k|
        b_2 = (1 - b_0) - b_1              db_0 + db_1 + U |1 - b_0| + U |b_2|
        z   = (b_0 z_0 + b_1 z_1) + b_2 z_2   sum db_k |z_k| + 3U sum |b_k z_k|     (w likewise)
        z/w                                dz / |w| + |z| dw / w^2 + U |z / w|

    In units of U (|a_0| + |a_1| + |a_2|) / |s| -- the condition of the quotient -- this is a small constant plus the cancellation
    of p_k = x_k - f w_k, 4 |w_k| / |p_k|, which the float64 values carry into the bound.  The clamps are 1-Lipschitz.  Second-order
    terms are covered by the factor 1.001.  Returns (bound of u and v [n, 2], bound of z/w [n], condition [n]) at the covered
    pixels, in the order of ``np.nonzero``."""
    H, W = keys.shape
    ids = F.ids_of(keys)
    jj, ii = np.nonzero(ids >= 0)
    v = p[tri[ids[jj, ii]]]
    fx, fy = (ii + 0.5) / W * 2 - 1, (jj + 0.5) / H * 2 - 1
    w = np.abs(v[:, :, 3])
    px, py = v[:, :, 0] - fx[:, None] * v[:, :, 3], v[:, :, 1] - fy[:, None] * v[:, :, 3]
    dpx, dpy = 4 * U * w + U * np.abs(px), 4 * U * w + U * np.abs(py)
    a, da = [], []
    for k in range(3):
        m, n = (k + 1) % 3, (k + 2) % 3
        t1, t2 = px[:, m] * py[:, n], py[:, m] * px[:, n]
        a.append(t1 - t2)
        da.append(dpx[:, m] * np.abs(py[:, n]) + np.abs(px[:, m]) * dpy[:, n] + dpy[:, m] * np.abs(px[:, n]) + np.abs(py[:, m]) * dpx[:, n]
                  + U * (np.abs(t1) + np.abs(t2)) + U * np.abs(t1 - t2))
    mass = np.abs(a[0]) + np.abs(a[1]) + np.abs(a[2])
    s = a[0] + a[1] + a[2]
    ds = da[0] + da[1] + da[2] + 2 * U * mass
    b = [a[k] / s for k in range(2)]
    db = [da[k] / np.abs(s) + np.abs(a[k]) * ds / s ** 2 + U * np.abs(b[k]) for k in range(2)]
    b.append(1 - b[0] - b[1])
    db.append(db[0] + db[1] + U * np.abs(1 - b[0]) + U * np.abs(b[2]))
    z, wq, dz, dw = 0.0, 0.0, 0.0, 0.0
    for k in range(3):
        z, wq = z + b[k] * v[:, k, 2], wq + b[k] * v[:, k, 3]
        dz = dz + db[k] * np.abs(v[:, k, 2]) + 3 * U * np.abs(b[k] * v[:, k, 2])
        dw = dw + db[k] * np.abs(v[:, k, 3]) + 3 * U * np.abs(b[k] * v[:, k, 3])
    dq = dz / np.abs(wq) + np.abs(z) * dw / wq ** 2 + U * np.abs(z / wq)
    return 1.001 * np.stack(db[:2], axis=1), 1.001 * dq, mass / np.abs(s)


def test_float32_statement_agrees_with_the_float64_oracle_within_its_rounding_bound():
    pos, tri, v = _kuhn4_scene()
    res = (48, 64)
    r32, zero_sign, keys = oracle_rast(pos, tri, res)
    worst_uv = worst_z = worst_cond = 0.0
    for b in range(pos.shape[0]):
        r64 = R.resolve(pos[b], tri, keys[b])
        hit = keys[b] != NO
        assert hit.mean() > 0.02
        assert np.array_equal(r32[b][~hit], np.zeros_like(r32[b][~hit])) and np.array_equal(r32[b, ..., 3].astype(np.float64), r64[..., 3])
        buv, bz, cond = _uv_bound(pos[b].astype(np.float64), tri.astype(np.int64), keys[b])
        euv = np.abs(r32[b][hit][:, :2].astype(np.float64) - r64[hit][:, :2])
        ez = np.abs(r32[b][hit][:, 2].astype(np.float64) - r64[hit][:, 2])
        worst_uv, worst_z = max(worst_uv, float((euv / buv).max())), max(worst_z, float((ez / bz).max()))
        worst_cond = max(worst_cond, float((euv.max(axis=1) / (U * cond)).max()))
        assert np.all(euv <= buv) and np.all(ez <= bz)
    print(f"float32 statement against float64: max error / bound {worst_uv:.3f} (u, v) {worst_z:.3f} (z/w); max error of (u, v) = "
          f"{worst_cond:.1f} U (|a0| + |a1| + |a2|) / |s|")
    assert worst_uv > 1e-3                                                        # the bound is not vacuous
    # interpolate: w = (1 - u) - v (2U), three products and two sums: 2U |a2| + 3U (|u a0| + |v a1| + |w a2|)
    rng = np.random.default_rng(3)
    attr = rng.standard_normal((2, v.shape[0], 3)).astype(np.float32)
    o32, o64 = F.interpolate32(attr, r32, tri), R.interpolate(attr, r32, tri)
    A = np.abs(attr.astype(np.float64))
    mag = R.interpolate(A, r32, tri) + 0.0
    bound = 3 * U * mag + 2 * U * np.abs(attr).max() + 1e-300
    assert np.all(np.abs(o32 - o64) <= 1.001 * bound)
    g = rng.standard_normal(o32.shape).astype(np.float32)
    gr32, (hit, ab, tt, terms) = F.interpolate_backward32(attr, r32, tri, g)
    ga64, gr64 = R.interpolate_backward(attr, r32, tri, g)
    assert np.abs(gr32 - gr64).max() <= 16 * U * np.abs(gr64).max()
    ok, _, zero_ok = F.any_order_sum_check(ga64, F.scatter_index(ab, tt, attr.shape[1], 3, np.arange(3)).reshape(-1), terms.reshape(-1), attr.shape)
    assert zero_ok and hit.sum() == (keys != NO).sum()
    assert np.abs(np.bincount(F.scatter_index(ab, tt, attr.shape[1], 3, np.arange(3)).reshape(-1), terms.reshape(-1).astype(np.float64),
                              minlength=attr.size).reshape(attr.shape) - ga64).max() <= 8 * U * np.abs(ga64).max()
    # rasterize_backward: the per-pixel contributions, summed in float64, against the float64 quotient rule
    gu = np.zeros_like(r32)
    gu[..., :2] = rng.standard_normal(r32.shape[:3] + (2,)).astype(np.float32)
    bb, tv, d = F.rasterize_backward32(pos, tri, r32, gu)
    gp64 = R.rasterize_backward(pos, tri, r32, gu)
    total = np.zeros(pos.shape)
    for k in range(3):
        for c, col in enumerate((0, 1, 3)):
            np.add.at(total[..., col], (bb, tv[:, k]), d[:, 3 * k + c].astype(np.float64))
    assert np.abs(total - gp64).max() <= 2e-3 * np.abs(gp64).max() and (total[..., 2] == 0).all()


# ------------------------------------------------ B.2 interpolate and grad_rast, bit for bit ------------------------------------------------

def _foreign_rast(B, H, W, n_tri, rng):
    """A hand-made ``rast``: arbitrary float (u, v), ids inside the list, beyond it, 0, negative, NaN, inf and 2^24."""
    rast = np.zeros((B, H, W, 4), dtype=np.float32)
    rast[..., :2] = rng.uniform(-0.25, 1.25, (B, H, W, 2)).astype(np.float32)
    rast[..., 2] = rng.uniform(-1, 1, (B, H, W)).astype(np.float32)
    ids = rng.integers(0, n_tri + 1, (B, H, W)).astype(np.float32)
    odd = rng.random((B, H, W))
    for lo, value in ((0.00, n_tri + 1.0), (0.03, n_tri + 7.0), (0.06, np.nan), (0.09, 2.0 ** 24), (0.12, 2.0 ** 24 + 2), (0.15, -3.0), (0.18, np.inf),
                      (0.21, 0.5), (0.24, 1.5)):
        ids[(odd >= lo) & (odd < lo + 0.03)] = value
    rast[..., 3] = ids
    return rast


@functools.lru_cache(maxsize=None)
def _interpolate_case(channels, attr_batch_is_one):
    rng = np.random.default_rng(10 * channels + attr_batch_is_one)
    B, H, W, V, T = 3, 7, 23, 30, 50                                     # 483 pixels: two workgroups, the second one ragged
    tri = rng.integers(0, V, (T, 3)).astype(np.int32)
    tri[5] = [0, 1, V]                                                   # vertex indices outside the attribute array
    tri[6] = [-1, 1, 2]
    rast = _foreign_rast(B, H, W, T, rng)
    attr = rng.standard_normal((1 if attr_batch_is_one else B, V, channels)).astype(np.float32)
    g = rng.standard_normal((B, H, W, channels)).astype(np.float32)
    return tri, rast, attr, g


@pytest.mark.parametrize("attr_batch_is_one", [True, False])
@pytest.mark.parametrize("channels", [1, 3, 4, 5])
def test_interpolate_fixture_holds_every_kind_of_pixel(channels, attr_batch_is_one):
    tri, rast, attr, g = _interpolate_case(channels, attr_batch_is_one)
    t = F.triangle_of(rast[..., 3], tri, attr.shape[1])
    w = rast[..., 3]
    assert (t >= 0).sum() > 100 and (t < 0).sum() > 100
    for bad in (np.isnan(w), w == 2.0 ** 24, w > 2.0 ** 24, w < 0, np.isinf(w), w == len(tri) + 1.0, (w > 0) & (w < 1), w == 6.0, w == 7.0):
        assert bad.any() and (t[bad] == -1).all()
    assert (t[w == 1.5] == 0).all() and (w == 1.5).any()                 # the id is truncated: 1.5 names triangle 0
    # and the float32 statement agrees with the float64 oracle on it (same background rules)
    o32, o64 = F.interpolate32(attr, rast, tri), R.interpolate(attr, rast, tri)
    assert np.abs(o32 - o64).max() <= 16 * U * max(1.0, np.abs(o64).max()) and np.array_equal(o32[t < 0], np.zeros_like(o32[t < 0]))


@pytest.mark.gpu
@pytest.mark.parametrize("attr_batch_is_one", [True, False])
@pytest.mark.parametrize("channels", [1, 3, 4, 5])
def test_interpolate_and_grad_rast_bit_exact(channels, attr_batch_is_one):
    import torch
    import tssplat_amd.dr as dr
    tri, rast_np, attr_np, g = _interpolate_case(channels, attr_batch_is_one)
    attr = torch.from_numpy(attr_np).cuda().requires_grad_(True)
    rast = torch.from_numpy(rast_np).cuda().requires_grad_(True)
    out, _ = dr.interpolate(attr, rast, torch.from_numpy(tri).cuda())
    out.backward(torch.from_numpy(g).cuda())
    want = F.interpolate32(attr_np, rast_np, tri)
    gr, (hit, ab, tt, terms) = F.interpolate_backward32(attr_np, rast_np, tri, g)
    assert F.same_bits(out.detach().cpu().numpy(), want)
    assert F.same_bits(rast.grad.cpu().numpy(), gr)
    index = F.scatter_index(ab, tt, attr_np.shape[1], channels, np.arange(channels)).reshape(-1)
    ok, ratio, zero_ok = F.any_order_sum_check(attr.grad.cpu().numpy(), index, terms.reshape(-1), attr_np.shape)
    print(f"grad_attr, {channels} channels, attr_batch {attr_np.shape[0]}: max error / any-order bound {ratio:.3f}")
    assert ok and zero_ok


# ------------------------------------------------ B.3 + C: runs of equal triangles in both backwards ------------------------------------------------

RUN_SHAPE = (3, 5, 40)                     # 600 pixels: 200 per view, rows of 40; 2 full workgroups + 88 pixels


@functools.lru_cache(maxsize=None)
def _runs_fixture():
    """Hand-made ids with the runs the wave scan has to get right.  Flat pixel g = 200 b + 40 y + x; a wave is 64 consecutive g."""
    B, H, W = RUN_SHAPE
    rng = np.random.default_rng(21)
    V, T = 12, 9
    tri = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11], [0, 4, 8], [1, 5, 9], [2, 6, 10], [3, 7, 11], [0, 5, 10]], dtype=np.int32)
    ids = rng.integers(0, T + 1, B * H * W)                             # 0 = background; runs of length 1 mostly
    ids[64:128] = 2                                                     # all 64 lanes of wave 1 (and three row wraps)
    ids[180:210] = 3                                                    # across the wave boundary at 192 AND the view boundary at 200
    ids[250:262] = 4                                                    # across the workgroup boundary at 256
    ids[395:405] = 5                                                    # the same triangle on both sides of the view boundary at 400
    ids[590:600] = 6                                                    # ends with the image, inside the ragged last workgroup
    ids[300:340] = 7                                                    # 40 lanes with zero-gradient lanes inside (below)
    zero = np.zeros(B * H * W, dtype=bool)
    zero[[70, 71, 185, 255, 310, 311, 312, 330, 599]] = True
    # exact data: (u, v) in eighths, integer attributes and gradients -- every product and partial sum is exact in float32
    u8 = rng.integers(0, 9, B * H * W)
    v8 = rng.integers(0, 9, B * H * W) % (9 - u8)
    rast = np.zeros((B * H * W, 4), dtype=np.float32)
    rast[:, 0], rast[:, 1], rast[:, 3] = u8 / 8.0, v8 / 8.0, ids
    rast[:, 2] = 0.25
    g = rng.integers(-8, 9, (B * H * W, 3)).astype(np.float32)
    g[zero] = 0.0
    attr = {1: rng.integers(-16, 17, (1, V, 3)).astype(np.float32), B: rng.integers(-16, 17, (B, V, 3)).astype(np.float32)}
    pts = rng.uniform(-1.0, 1.0, (B, V, 2))
    w = rng.uniform(0.6, 1.8, (B, V))
    pos = np.concatenate([pts * w[..., None], (rng.uniform(-0.8, 0.8, (B, V)) * w)[..., None], w[..., None]], axis=-1).astype(np.float32)
    return tri, ids.reshape(B, H, W), zero.reshape(B, H, W), rast.reshape(B, H, W, 4), g.reshape(B, H, W, 3), attr, pos


def _runs_of(keys):
    """``find_runs`` restated: (start, length) of every run of equal consecutive keys inside each 64-lane wave."""
    out = []
    for w0 in range(0, len(keys), 64):
        k = keys[w0:w0 + 64]
        start = 0
        for i in range(1, len(k) + 1):
            if i == len(k) or k[i] != k[start]:
                out.append((w0 + start, i - start))
                start = i
    return out


def test_runs_fixture_reaches_every_run_edge():
    tri, ids, zero, rast, g, attr, pos = _runs_fixture()
    B, H, W = RUN_SHAPE
    assert (B * H * W) % 256 != 0 and (B * H * W) % 64 != 0
    flat = ids.reshape(-1).astype(np.int64)
    view = np.arange(B * H * W) // (H * W)
    lane_unique = -1 - np.arange(B * H * W)
    # interpolate_backward, attr_batch == 1: key = triangle (background lanes are their own run)
    shared = _runs_of(np.where(flat > 0, flat, lane_unique))
    assert (64, 64) in shared                                           # a run of all 64 lanes
    assert (180, 12) in shared and (192, 18) in shared                  # across a wave: cut at 192, and MERGED across the view boundary at 200
    assert (250, 6) in shared and (256, 6) in shared                    # across a workgroup
    assert (395, 10) in shared                                          # merged across the view boundary at 400 (same attribute row: allowed)
    assert (590, 10) in shared and (300, 20) in shared and (320, 20) in shared
    # interpolate_backward with attr_batch == B and rasterize_backward: key = (view, triangle)
    per_view = _runs_of(np.where(flat > 0, view * (1 << 32) + flat, lane_unique))
    assert (192, 8) in per_view and (200, 10) in per_view and (395, 5) in per_view and (400, 5) in per_view
    # rasterize_backward drops zero-gradient lanes: they cut the runs around them
    valid = (flat > 0) & ~zero.reshape(-1)
    cut = _runs_of(np.where(valid, view * (1 << 32) + flat, lane_unique))
    assert (64, 6) in cut and (72, 56) in cut and (300, 10) in cut and (313, 7) in cut and (320, 10) in cut    # (72, 56): longer than half a wave
    assert (192, 8) in cut and (200, 10) in cut and (395, 5) in cut and (400, 5) in cut      # valid lanes on both sides of a view boundary
    assert any(s // W != (s + n - 1) // W and n > 1 for s, n in cut)    # a run that wraps a row
    # the data are exact: every partial sum of the scatter is an integer number of eighths below 2^24
    for a in attr.values():
        _, (hit, ab, tt, terms) = F.interpolate_backward32(a, rast, tri, g)
        t64 = np.stack([rast[..., k][hit][:, None].astype(np.float64) * g[hit] for k in (0, 1)], axis=1)
        assert np.array_equal(terms[:, :2].astype(np.float64), t64) and np.array_equal(terms * 8, np.round(terms * 8))
        mass = np.zeros(a.size)
        np.add.at(mass, F.scatter_index(ab, tt, a.shape[1], 3, np.arange(3)).reshape(-1), np.abs(terms.reshape(-1)).astype(np.float64))
        assert mass.max() * 8 < 2 ** 24 and mass.max() > 50


def _exact_grad_attr(a, rast, tri, g):
    _, (hit, ab, tt, terms) = F.interpolate_backward32(a, rast, tri, g)
    want = np.bincount(F.scatter_index(ab, tt, a.shape[1], 3, np.arange(3)).reshape(-1), terms.reshape(-1).astype(np.float64), minlength=a.size)
    return want.reshape(a.shape).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("attr_batch_is_one", [True, False])
def test_runs_grad_attr_bit_exact_on_exact_data(attr_batch_is_one):
    import torch
    import tssplat_amd.dr as dr
    tri, ids, zero, rast_np, g, attrs, pos = _runs_fixture()
    a = attrs[1 if attr_batch_is_one else RUN_SHAPE[0]]
    attr = torch.from_numpy(a).cuda().requires_grad_(True)
    rast = torch.from_numpy(rast_np).cuda().requires_grad_(True)
    out, _ = dr.interpolate(attr, rast, torch.from_numpy(tri).cuda())
    out.backward(torch.from_numpy(g).cuda())
    assert F.same_bits(out.detach().cpu().numpy(), F.interpolate32(a, rast_np, tri))
    assert F.same_bits(rast.grad.cpu().numpy(), F.interpolate_backward32(a, rast_np, tri, g)[0])
    assert np.array_equal(attr.grad.cpu().numpy(), _exact_grad_attr(a, rast_np, tri, g))


def _check_grad_pos(pos, tri, rast, grad_rast, got, label):
    bb, tv, d = F.rasterize_backward32(pos, tri, rast, grad_rast)
    V = pos.shape[1]
    index = F.scatter_index(bb, tv, V, 4, np.array([0, 1, 3])).reshape(-1)
    ok, ratio, zero_ok = F.any_order_sum_check(got, index, d.reshape(-1, 3, 3).reshape(-1), pos.shape)
    print(f"grad_pos, {label}: {len(bb)} contributing pixels, max error / any-order bound {ratio:.3f}")
    assert len(bb) > 50 and ok and zero_ok and np.isfinite(got).all()


@pytest.mark.gpu
def test_runs_grad_pos_within_the_any_order_bound():
    import torch
    from tssplat_amd import _capi
    lib = _capi.load()
    tri, ids, zero, rast_np, g, attrs, pos = _runs_fixture()
    B, H, W = RUN_SHAPE
    gr = np.zeros_like(rast_np)
    gr[..., :2] = np.random.default_rng(5).standard_normal((B, H, W, 2)).astype(np.float32)
    gr[zero] = 0.0
    gr[..., 2:] = 7.0                                                 # (z/w and the id carry no gradient: ignored)
    d = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (pos, tri, rast_np, gr)]
    out = torch.full((B, pos.shape[1], 4), float("nan"), device="cuda")
    _capi.check(lib.tsamd_rasterize_backward(d[0].data_ptr(), B, pos.shape[1], d[1].data_ptr(), tri.shape[0], H, W, d[2].data_ptr(), d[3].data_ptr(),
                                             out.data_ptr(), None))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[..., 2] == 0).all()
    _check_grad_pos(pos, tri, rast_np, gr, got, "runs fixture")


@pytest.mark.gpu
def test_random_scene_gradients_within_the_any_order_bound():
    """B.3(b) on a rendered scene: rasterize -> interpolate -> backward; grad_attr and grad_pos against the float32 per-pixel
    contributions summed in float64, |got - sum c_i| <= gamma_(n-1) sum |c_i| per vertex component."""
    import torch
    import tssplat_amd.dr as dr
    pos_np, tri, v = _kuhn4_scene()
    res = (48, 64)
    tri_d = torch.from_numpy(tri).cuda()
    pos = torch.from_numpy(pos_np).cuda().requires_grad_(True)
    attr_np = np.random.default_rng(8).standard_normal((1, v.shape[0], 3)).astype(np.float32)
    attr = torch.from_numpy(attr_np).cuda().requires_grad_(True)
    rast, _ = dr.rasterize(dr.RasterizeCudaContext(), pos, tri_d, resolution=list(res), grad_db=False)
    out, _ = dr.interpolate(attr, rast, tri_d)
    g = np.random.default_rng(9).standard_normal(tuple(out.shape)).astype(np.float32)
    out.backward(torch.from_numpy(g).cuda())
    rast_np = rast.detach().cpu().numpy()
    want, zero_sign, _ = oracle_rast(pos_np, tri, res)
    assert F.same_bits(rast_np, want)
    gr, (hit, ab, tt, terms) = F.interpolate_backward32(attr_np, rast_np, tri, g)
    index = F.scatter_index(ab, tt, attr_np.shape[1], 3, np.arange(3)).reshape(-1)
    ok, ratio, zero_ok = F.any_order_sum_check(attr.grad.cpu().numpy(), index, terms.reshape(-1), attr_np.shape)
    print(f"grad_attr, kuhn4 scene: {int(hit.sum())} contributing pixels, max error / any-order bound {ratio:.3f}")
    assert ok and zero_ok
    _check_grad_pos(pos_np, tri, rast_np, gr, pos.grad.cpu().numpy(), "kuhn4 scene")


# ------------------------------------------------ C. tiny images: resolve and cover below 256 pixels ------------------------------------------------

TINY_SHAPES = [(1, 1), (1, 3), (3, 5), (15, 17), (16, 16), (1, 257), (257, 1), (5, 13)]
TINY_BATCHES = [1, 2, 5, 70]
TINY_EXTRA = [(21, (1, 3)), (64, (1, 1)), (1, (7, 9)), (1, (8, 8)), (4, (8, 8))]      # B H W = 63, 64, 63, 64; lane 63 at a last column
TINY_CASES = [(b, s) for s in TINY_SHAPES for b in TINY_BATCHES] + TINY_EXTRA


@functools.lru_cache(maxsize=None)
def _tiny_scene(batch):
    rng = np.random.default_rng(100 + batch)
    V, T = 18, 12
    pts = rng.uniform(-1.4, 1.4, (batch, V, 2))
    w = rng.uniform(0.5, 2.0, (batch, V))
    pos = np.concatenate([pts * w[..., None], (rng.uniform(-0.9, 0.9, (batch, V)) * w)[..., None], w[..., None]], axis=-1).astype(np.float32)
    tri = rng.integers(0, V, (T, 3)).astype(np.int32)
    return pos, tri


def test_tiny_image_table_reaches_the_small_image_path():
    sizes = {b * h * w for b, (h, w) in TINY_CASES}
    assert {63, 64, 65, 255, 256, 257} <= sizes
    assert any(h * w < 256 and b * h * w > 256 for b, (h, w) in TINY_CASES)                   # a wave over several views, more than one wave
    assert any(h * w < 256 and -(-256 // (h * w)) >= 70 for b, (h, w) in TINY_CASES if b == 70)   # ... over all 70 views
    assert any(h * w == 256 for _, (h, w) in TINY_CASES) and any(h * w == 255 for _, (h, w) in TINY_CASES)
    assert any(w == 1 for _, (h, w) in TINY_CASES) and any(h == 1 for _, (h, w) in TINY_CASES)
    assert any(64 % w == 0 and h * w >= 64 and w > 1 for _, (h, w) in TINY_CASES)              # flat pixel 63 is the last pixel of a row
    covered = background = pairs = 0
    for b, res in TINY_CASES:
        pos, tri = _tiny_scene(b)
        rast, _, keys = oracle_rast(pos, tri, res)
        covered, background = covered + int((keys != NO).sum()), background + int((keys == NO).sum())
        if res == (16, 16):
            flat = F.ids_of(keys).reshape(b, -1)
            assert (flat[:, 63:-1:64] != flat[:, 64::64]).any()              # lane 63 | the next row's first pixel differ: the column guard matters
        if res[0] * res[1] >= 15 and b * res[0] * res[1] >= 60:
            assert (keys != NO).any() and pair_masks_of(F.ids_of(keys)).any()
            pairs += int(SO.coverage_pairs(rast).sum())
    assert covered > 5000 and background > 5000 and pairs > 1000


@pytest.mark.gpu
@pytest.mark.parametrize("batch,res", TINY_CASES)
def test_tiny_images_bit_exact(batch, res):
    pos, tri = _tiny_scene(batch)
    check_device(pos, tri, res, full_alpha=True)


# The resolve pass WITHOUT pair masks, in every placement regime of a wave of 4 x 64 pixels: several views per wave (H W < 256), a wave
# that straddles one view boundary, full chunks only, a wave that ends in mid-row (where the masked pass makes its extra load of the
# right-hand key), a short last wave.  (With masks, and for the cover pass, test_tiny_images_bit_exact reaches all five.)
NO_MASK_CASES = [(5, (6, 8)), (5, (8, 8)), (3, (33, 50)), (1, (32, 32)), (2, (7, 192))]


@pytest.mark.gpu
@pytest.mark.parametrize("batch,res", NO_MASK_CASES)
def test_resolve_without_masks_bit_exact(batch, res):
    pos, tri = _tiny_scene(batch)
    want, zero_sign, keys = oracle_rast(pos, tri, res)
    got_keys, got, masks = device_rasterize(pos, tri, res, want_masks=False)
    assert np.array_equal(got_keys, keys)
    assert F.same_bits(got, want), f"{int(zero_sign.sum())} pixels with a -0 barycentric"
    assert (masks.view(np.uint8) == 0xAB).all()                                                # nothing was written through a null pointer's twin


# ------------------------------------------------ C. the fragment queue of the pixel walk ------------------------------------------------

QUEUE = 320                                                            # kQueue of raster_kernels.hip; drained when count > QUEUE - 64


def walk_counts(pos_b, tri, res, wave):
    """Emulator of ``wave_walk``'s counting for the 64 consecutive triangles of wave ``wave`` (of one view): what every iteration of
    the wave-uniform loop appends to the LDS queue, derived from the oracle's coverage.  A lane steps through the pixel centres of
    its triangle's bounding box, row by row; it appends where the oracle (the triangle rasterised alone) has a fragment.  The
    32-bit walk (reach < 2^14) runs first, the 64-bit walk after it, the queue's count carried over; the queue is drained when
    ``count > QUEUE - 64`` after an append, and once at the end.
    Returns ``(appended per appending iteration, count at every mid-walk drain, count at the final drain, covering lanes, peak count)``."""
    H, W = res
    X, Y, _, ok = R.snap_vertices(pos_b, H, W)
    lanes = {True: [], False: []}
    for t in range(64 * wave, min(64 * wave + 64, len(tri))):
        i = tri[t]
        if not ok[i].all():
            continue                                                   # dropped, or left to the clip kernel
        xs, ys = [int(X[k]) for k in i], [int(Y[k]) for k in i]
        if (xs[1] - xs[0]) * (ys[2] - ys[0]) - (ys[1] - ys[0]) * (xs[2] - xs[0]) == 0:
            continue
        px0, px1 = max(0, (min(xs) - 128 + 255) // 256), min(W - 1, (max(xs) - 128) // 256)
        py0, py1 = max(0, (min(ys) - 128 + 255) // 256), min(H - 1, (max(ys) - 128) // 256)
        if px0 > px1 or py0 > py1:
            continue
        cov = R.rasterize_ids(pos_b, tri[t:t + 1], H, W) != NO
        assert not cov.any() or (cov[py0:py1 + 1, px0:px1 + 1].sum() == cov.sum())
        reach = max(max(abs(xs[a] - xs[b]), abs(ys[a] - ys[b])) for a, b in ((0, 1), (1, 2), (2, 0)))
        lanes[reach < (1 << 14)].append(cov[py0:py1 + 1, px0:px1 + 1].reshape(-1))
    appended, drains, count, peak = [], [], 0, 0
    for small in (True, False):
        seqs = lanes[small]
        for k in range(max([len(s) for s in seqs], default=0)):
            add = sum(int(s[k]) for s in seqs if k < len(s))
            if add:
                appended.append(add)
                count += add
                peak = max(peak, count)
                if count > QUEUE - 64:
                    drains.append(count)
                    count = 0
    covering = sum(int(s.any()) for s in lanes[True] + lanes[False])
    return appended, drains, count, covering, peak


@functools.lru_cache(maxsize=None)
def _queue_fixture():
    """256 triangles = the four waves of one workgroup, on a 256 x 64 image.
    wave 0: 64 congruent right triangles (6 x 20 pixels, their two lowest rows fully inside): every lane appends in each of the first
            12 iterations -- 64, 128, .., 320 -> the mid-walk drain fires with count == 320;
    wave 1: ONE covering lane with more than 256 fragments (drains mid-walk at 257), the other lanes degenerate or off screen;
    wave 2: one covering lane with 192 < fragments <= 256: the final drain runs its base loop twice;
    wave 3: a few small triangles: the final drain runs once."""
    res = (256, 64)
    pts, tri = [], []

    def add(tr, z):
        k = len(pts)
        pts.extend([(x, y, z) for x, y in tr])
        tri.append([k, k + 1, k + 2])

    for i in range(64):
        x0, y0 = 256 * 8 * (i % 8), 256 * 32 * (i // 8)
        add([(x0, y0), (x0 + 6 * 256, y0), (x0, y0 + 20 * 256)], 0.5 - i / 256.0)
    for wave, legs in ((1, (24, 26)), (2, (21, 22))):
        for lane in range(64):
            if lane == 37:
                add([(300, 300 + 30 * 256 * (wave - 1)), (300 + legs[0] * 256, 300 + 30 * 256 * (wave - 1)), (300, 300 + (30 * (wave - 1) + legs[1]) * 256)], -0.25 * wave)
            elif lane % 3 == 0:
                add([(lane * 256, 40), (lane * 256 + 40, 40), (lane * 256 + 80, 40)], 0.0)                   # zero area
            elif lane % 3 == 1:
                add([(-5000 - lane, 200), (-3000, 200), (-4000, 900)], 0.0)                                    # off screen
            else:
                add([(lane * 256 + 130, 130), (lane * 256 + 250, 130), (lane * 256 + 130, 250)], 0.0)          # between pixel centres
    for lane in range(64):
        x0, y0, leg = lane * 200 + 50, 40000 + lane * 300, 650 if lane < 40 else 0
        add([(x0, y0), (x0 + leg, y0), (x0, y0 + leg)], 0.7 - lane / 128.0)
    return subpixel_vertices(pts, res)[None], np.array(tri, dtype=np.int32), res


def test_queue_fixture_drains_mid_walk_and_twice_at_the_end():
    pos, tri, res = _queue_fixture()
    assert tri.shape[0] == 256
    w = [walk_counts(pos[0], tri, res, k) for k in range(4)]
    appended, drains, final, covering, peak = w[0]
    assert covering == 64 and appended[:12] == [64] * 12 and drains[0] == 320 and len(drains) >= 2 and peak == QUEUE
    appended, drains, final, covering, peak = w[1]
    assert covering == 1 and set(appended) == {1} and drains == [257] and 1 <= final <= 192
    appended, drains, final, covering, peak = w[2]
    assert covering == 1 and drains == [] and 192 < final <= 256                        # the final drain's base loop runs twice
    appended, drains, final, covering, peak = w[3]
    assert covering > 3 and drains == [] and 1 <= final <= 192
    # the queue never holds more than its 320 entries: a drain at `count > 320 - 63` instead would let 257 + 64 = 321 in
    assert all(k[4] <= QUEUE for k in w) and max(k[4] for k in w) == QUEUE
    assert all(d <= QUEUE for k in w for d in k[1]) and (QUEUE - 63) + 64 > QUEUE
    # and everything appended is a winner or hidden: the oracle's image shows all four waves
    ids = F.ids_of(oracle_keys(pos, tri, res))
    assert all(((ids >= 64 * k) & (ids < 64 * k + 64)).any() for k in range(4))


@pytest.mark.gpu
def test_queue_fixture_bit_exact():
    check_device(*_queue_fixture())


# ------------------------------------------------ C. the 32-bit | 64-bit walk switch ------------------------------------------------

@functools.lru_cache(maxsize=None)
def _walk_switch_fixture():
    """Three triangles of one wave on a 32 x 32 image (8192 sub-pixel units): largest edge component 16383 (the last 32-bit walk),
    16384 (the first 64-bit walk), and 16383 with a vertex beyond the left and lower side and its long edge across the right and upper one."""
    res = (32, 32)
    pts = [(100, 100, 0.0), (16483, 100, 0.0), (100, 5100, 0.0),
           (-9000, 2000, -0.5), (7384, 2000, -0.5), (-9000, 8000, -0.5),
           (-4000, -4000, 0.5), (12383, -4000, 0.5), (-4000, 12383, 0.5)]
    return subpixel_vertices(pts, res)[None], np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]], dtype=np.int32), res


def _reach(pos_b, tri_row, res):
    X, Y, _, ok = R.snap_vertices(pos_b, *res)
    assert ok[tri_row].all()
    return max(max(abs(int(X[a] - X[b])), abs(int(Y[a] - Y[b]))) for a, b in ((tri_row[0], tri_row[1]), (tri_row[1], tri_row[2]), (tri_row[2], tri_row[0])))


def test_walk_switch_fixture_sits_on_both_sides_of_2_to_14():
    pos, tri, res = _walk_switch_fixture()
    assert [_reach(pos[0], t, res) for t in tri] == [16383, 16384, 16383]
    X, Y, _, _ = R.snap_vertices(pos[0], *res)
    assert X[tri[2]].min() < 0 and Y[tri[2]].min() < 0 and X[tri[2]].max() > 8192 and Y[tri[2]].max() > 8192
    alone = R.rasterize_ids(pos[0], tri[2:], *res) != NO
    assert alone[0].any() and alone[-1].any() and alone[:, 0].any() and alone[:, -1].any() and not alone.all()   # touches all four sides, leaves a corner out
    ids = F.ids_of(oracle_keys(pos, tri, res))
    assert all((ids == t).sum() > 20 for t in range(3))
    # |E| stays below 2^31 at reach 2^14 (2 * 2^14 * (2^14 + 2^8)): the two walks hold the same integers there -- the switch is about
    # WHICH walk a triangle takes, and that each takes exactly one
    assert 2 * 16384 * (16384 + 256) < 2 ** 31


@pytest.mark.gpu
def test_walk_switch_bit_exact():
    check_device(*_walk_switch_fixture())


# ------------------------------------------------ C. snap: guard band, half-way rounding, w at the edge of the numbers ------------------------------------------------

@functools.lru_cache(maxsize=None)
def _snap_fixture():
    """64 x 64.  Triangles 0-3: one vertex at X or Y = +-2^22 (kept, the 64-bit walk); 4-7: the same at +-(2^22 + 1) (dropped), nearer
    than everything, so a kept one would hide the rest.  8: left and lower edge at sub-pixel 128.5 -> 129 (round half up), off pixel
    0's centre.  9: a vertex with a subnormal w far off the guard band (dropped).  10: a subnormal w under a zero (x, y, z): kept.
    11, 12: w = -0.0 and +0.0 (finite, not in front: the clip path).  13-20: +-inf in each component (dropped).
    21: clip coordinates scaled by 2^-80: every edge function underflows to 0 -- the s == 0 guard of the resolve pass."""
    res = (64, 64)
    big = LIMIT
    pts, tri, extra = [], [], []

    def add(tr, z):
        k = len(pts)
        pts.extend([(x, y, z) for x, y in tr])
        tri.append([k, k + 1, k + 2])

    for far, z in ((big, 0.5), (big + 1, -0.9)):
        add([(far, 8192), (1000, 12000), (1000, 4000)], z)
        add([(-far, 8192), (15000, 4000), (15000, 12000)], z + 0.01)
        add([(8192, far), (4000, 1000), (12000, 1000)], z + 0.02)
        add([(8192, -far), (12000, 15000), (4000, 15000)], z + 0.03)
    add([(128.5, 128.5), (2000.5, 128.5), (128.5, 2000.5)], -0.5)
    pos = subpixel_vertices(pts, res)
    n = len(pos)
    tiny = np.float32(2.0 ** -140)
    assert 0 < tiny < np.finfo(np.float32).tiny
    base = np.array([[-0.5, -0.5, 0.1, 1.0], [0.5, -0.5, 0.1, 1.0]], dtype=np.float32)
    special = [np.array([0.25, 0.5, 0.1, tiny], dtype=np.float32), np.array([0.0, 0.5, 0.1, 1.0], dtype=np.float32),
               np.array([0.0, 0.5, -0.3, -0.0], dtype=np.float32), np.array([0.0, 0.5, 0.3, 0.0], dtype=np.float32)]
    for c in range(4):
        for sign in (1.0, -1.0):
            v = np.array([0.0, 0.5, 0.1, 1.0], dtype=np.float32)
            v[c] = sign * np.inf
            special.append(v)
    rows = [base[0], base[1]] + special
    tri += [[n, n + 1, n + 2 + k] for k in range(len(special))]
    scaled = (np.array([[-0.75, 0.5, 0.3, 1.0], [-0.25, 0.5, 0.3, 1.0], [-0.5, 0.9, 0.3, 1.0]]) * 2.0 ** -80).astype(np.float32)
    tri.append([n + len(rows), n + len(rows) + 1, n + len(rows) + 2])
    own = np.array([[0.3, -0.9, -0.6, 1.0], [0.9, -0.9, -0.6, 1.0], [0.0, 0.0, 0.0, tiny]], dtype=np.float32)     # triangle 10's
    tri[10] = [n + len(rows) + 3, n + len(rows) + 4, n + len(rows) + 5]
    pos = np.concatenate([pos, np.stack(rows), scaled, own]).astype(np.float32)
    return pos[None], np.array(tri, dtype=np.int32), res


def _oracle_dropped(pos, tri, res):
    n = 0
    for b in range(pos.shape[0]):
        _, _, _, ok = R.snap_vertices(pos[b], *res)
        p = pos[b].astype(np.float64)
        fine = ok | (np.isfinite(p).all(axis=1) & (p[:, 3] <= 0.0))
        n += int((~fine[tri].all(axis=1)).sum())
    return n


def test_snap_fixture_reaches_the_guard_band_and_the_rounding():
    pos, tri, res = _snap_fixture()
    X, Y, ZW, ok = R.snap_vertices(pos[0], *res)
    assert [int(X[tri[0, 0]]), int(X[tri[1, 0]]), int(Y[tri[2, 0]]), int(Y[tri[3, 0]])] == [LIMIT, -LIMIT, LIMIT, -LIMIT] and ok[tri[:4, 0]].all()
    assert not ok[tri[4:8, 0]].any() and ok[tri[4:8, 1:]].all()
    p64 = pos[0].astype(np.float64)
    for k, axis in zip(range(4, 8), (0, 0, 1, 1)):                       # exactly one unit beyond: the rounded coordinate is 2^22 + 1
        q = p64[tri[k, 0]]
        assert abs(np.floor(((q[axis] * 0.5 + 0.5) * 64.0) * 256.0 + 0.5)) == LIMIT + 1
    assert (int(X[tri[8, 0]]), int(Y[tri[8, 0]])) == (129, 129) and ((p64[tri[8, 0], 0] * 0.5 + 0.5) * 64 * 256 == 128.5)
    ids = F.ids_of(oracle_keys(pos, tri, res))
    seen = set(np.unique(ids).tolist())
    assert {0, 1, 2, 3, 8, 10, 21} <= seen and not seen & ({4, 5, 6, 7, 9} | set(range(13, 21)))
    assert ids[0, 0, 0] != 8 and ids[0, 1, 1] == 8                             # 129 is past pixel 0's centre (128); a floor or half-even snap keeps it
    assert not ok[tri[9, 2]] and ok[tri[10, 2]] and 0 < pos[0, tri[10, 2], 3] < np.finfo(np.float32).tiny and not ok[tri[11, 2]] and not ok[tri[12, 2]]
    # the scaled triangle: float32 edge functions underflow to zero, s == 0 -> 1, (u, v) = (0, 0), z/w of the third vertex
    rast, _, keys = oracle_rast(pos, tri, res)
    at = ids == 21
    assert at.sum() > 10 and (rast[at][:, :2] == 0).all() and np.array_equal(rast[at][:, 2], np.full(at.sum(), np.float32(0.3), dtype=np.float32))
    assert _oracle_dropped(pos, tri, res) == 4 + 1 + 8


@pytest.mark.gpu
def test_snap_fixture_bit_exact():
    import torch
    import tssplat_amd.dr as dr
    pos, tri, res = _snap_fixture()
    check_device(pos, tri, res)
    assert dr.count_dropped_triangles(torch.from_numpy(pos).cuda(), torch.from_numpy(tri).cuda(), *res) == _oracle_dropped(pos, tri, res)


def test_dropped_triangle_counter_agrees_with_the_oracle_on_the_snap_fixture():
    import torch
    import tssplat_amd.dr as dr
    pos, tri, res = _snap_fixture()
    assert dr.count_dropped_triangles(torch.from_numpy(pos), torch.from_numpy(tri), *res) == _oracle_dropped(pos, tri, res)


# ------------------------------------------------ C. depth: the limits of z/w and equal keys ------------------------------------------------

@functools.lru_cache(maxsize=None)
def _depth_fixture():
    """Eight views of three full-screen quads A (triangles 0, 1), B (2, 3), Z (4, 5 = the highest ids); z = 5 parks a quad beyond the
    far plane.  z/w is constant per quad, so every pixel holds the same depth.
      0: A at -1 (depth 0)                      1: A at +1 ((z + 1) 2^31 = 2^32: clamped to 0xFFFFFFFF)
      2: A one float32 step below -1 (dropped)  3: A one step above +1 (dropped)
      4: A and B both at -1 (coplanar duplicates: the lower id)
      5: A one step above -1 (depth 128), Z at -1 (depth 0): the nearer plane, whatever its id
      6: A at +1, B one step below (1 - 2^-24): z + 1 rounds to 2, both clamp to 0xFFFFFFFF -- merged, the lower id wins though B is nearer
      7: A and Z at 0.25: id 0 against the highest id at equal depth
    (Near -1 a float32 z/w is a multiple of 2^-25, so (z + 1) 2^31 is an integer there: the truncation to uint32 cannot merge two
    planes at that end; what merges is the rounding of z + 1 and the clamp at the far end, view 6.)"""
    res = (16, 16)
    one = np.float32(1.0)
    below, above = np.nextafter(-one, np.float32(-2)), np.nextafter(one, np.float32(2))
    inside_lo, inside_hi = np.nextafter(-one, np.float32(0)), np.nextafter(one, np.float32(0))
    park = 5.0
    zs = [(-1, park, park), (1, park, park), (below, park, park), (above, park, park), (-1, -1, park), (inside_lo, park, -1), (1, inside_hi, park),
          (0.25, park, 0.25)]
    quad = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], dtype=np.float32)
    pos = np.zeros((len(zs), 12, 4), dtype=np.float32)
    for b, z3 in enumerate(zs):
        for q, z in enumerate(z3):
            pos[b, 4 * q:4 * q + 4, :2], pos[b, 4 * q:4 * q + 4, 2], pos[b, 4 * q:4 * q + 4, 3] = quad, z, 1.0
    tri = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7], [8, 9, 10], [8, 10, 11]], dtype=np.int32)
    return pos, tri, res


def test_depth_fixture_reaches_both_limits_and_every_tie():
    pos, tri, res = _depth_fixture()
    keys = oracle_keys(pos, tri, res)
    depth, ids = (keys >> np.uint64(32)).astype(np.int64), F.ids_of(keys)
    assert (depth[0] == 0).all() and np.isin(ids[0], [0, 1]).all()
    assert (depth[1] == 0xFFFFFFFF).all() and np.isin(ids[1], [0, 1]).all()
    assert (keys[2] == NO).all() and (keys[3] == NO).all()
    assert pos[2, 0, 2] < -1 and pos[3, 0, 2] > 1 and np.float32(pos[2, 0, 2]) == np.nextafter(np.float32(-1), np.float32(-2))
    assert (depth[4] == 0).all() and np.isin(ids[4], [0, 1]).all()
    assert (depth[5] == 0).all() and np.isin(ids[5], [4, 5]).all() and -1 < pos[5, 0, 2] < -1 + 1e-7
    assert (np.float32(pos[5, 0, 2]) + np.float32(1)) * np.float32(2.0 ** 31) == 128
    assert (depth[6] == 0xFFFFFFFF).all() and np.isin(ids[6], [0, 1]).all() and pos[6, 4, 2] < pos[6, 0, 2]
    assert np.isin(ids[7], [0, 1]).all() and len(tri) - 1 == 5
    for b in range(8):
        assert (keys[b] == NO).all() or {int(k) for k in np.unique(ids[b])} in ({0, 1}, {4, 5})


@pytest.mark.gpu
def test_depth_fixture_bit_exact():
    got = check_device(*_depth_fixture())
    assert (got[0, ..., 2] == -1).all() and (got[1, ..., 2] == 1).all() and (got[2:4] == 0).all()


# ------------------------------------------------ C. launch: triangle counts and the XCD-affine route ------------------------------------------------

LAUNCH_RES = (8, 8)
LAUNCH_CASES = [(1, 3), (255, 3), (256, 3), (257, 3), (513, 3), (255, 8), (256, 8), (257, 8), (513, 8), (257, 65)] + \
               [(70, b) for b in (7, 8, 9, 16, 63, 64, 65, 71)]          # (triangles, views)


def xcd_route(n_tri, batch, res):
    """``launch_depth_keys`` restated: (XCD-affine route taken, workgroups launched, workgroups that return at ``b >= n_views``)."""
    blocks_per_view = (n_tri + 255) // 256
    xcd = n_tri >= res[0] * res[1] and (batch % 8 == 0 or batch >= 64)
    views = (batch + 7) // 8 * 8 if xcd else batch
    return xcd, views * blocks_per_view, (views - batch) * blocks_per_view


@functools.lru_cache(maxsize=None)
def _launch_scene(n_tri, batch):
    rng = np.random.default_rng(1000 * n_tri + batch)
    V = 40
    pts = rng.uniform(-1.2, 1.2, (batch, V, 2))
    w = rng.uniform(0.5, 2.0, (batch, V))
    pos = np.concatenate([pts * w[..., None], (rng.uniform(-0.9, 0.9, (batch, V)) * w)[..., None], w[..., None]], axis=-1).astype(np.float32)
    c = rng.integers(0, V, n_tri)
    tri = np.stack([c, (c + rng.integers(1, 4, n_tri)) % V, (c + rng.integers(4, 9, n_tri)) % V], axis=1).astype(np.int32)
    return pos, tri


def test_launch_table_takes_both_routes_and_the_early_return():
    routes = {case: xcd_route(*case, LAUNCH_RES) for case in LAUNCH_CASES}
    assert {t for t, _ in LAUNCH_CASES} >= {1, 255, 256, 257, 513}
    on = {b for (t, b), r in routes.items() if r[0] and t == 70}
    off = {b for (t, b), r in routes.items() if not r[0] and t == 70}
    assert on == {8, 16, 64, 65, 71} and off == {7, 9, 63}
    assert routes[(70, 65)][2] == 7 and routes[(70, 71)][2] == 1 and routes[(257, 65)][2] == 14 and routes[(70, 64)][2] == 0
    assert routes[(513, 8)] == (True, 24, 0) and routes[(1, 3)][0] is False and routes[(513, 3)] == (False, 9, 0)
    for t, b in ((513, 8), (70, 71)):                                    # the scenes are in view, and the last triangle / last view too
        pos, tri = _launch_scene(t, b)
        ids = F.ids_of(oracle_keys(pos, tri, LAUNCH_RES))
        assert (ids >= 0).mean() > 0.3 and (ids[-1] >= 0).any() and len(np.unique(ids)) > 20
    pos, tri = _launch_scene(513, 8)
    assert (F.ids_of(oracle_keys(pos, tri, LAUNCH_RES)) >= 256).any()


@pytest.mark.gpu
@pytest.mark.parametrize("n_tri,batch", LAUNCH_CASES)
def test_launch_edges_bit_exact(n_tri, batch):
    pos, tri = _launch_scene(n_tri, batch)
    check_device(pos, tri, LAUNCH_RES)


# ------------------------------------------------ C. the clip kernel: flagged views around 64, triangles past the first trip ------------------------------------------------

def _ground_clip():
    near, far, f = 0.1, 50.0, 1.0 / np.tan(np.radians(30.0))
    proj = np.array([[f, 0, 0, 0], [0, f, 0, 0], [0, 0, (far + near) / (near - far), 2 * far * near / (near - far)], [0, 0, -1, 0]])
    view = np.eye(4)
    view[1, 3] = -1.0
    mvp = proj @ view
    return lambda v: (np.concatenate([v, np.ones((len(v), 1))], axis=1) @ mvp.T).astype(np.float32)


GROUND = np.array([[-30.0, 0, 8], [-10.0, 0, 8], [0.0, 0, 8], [10.0, 0, 8], [30.0, 0, 8], [0.0, 0, -40]])     # a fan on the ground
GROUND_TRI = np.array([[0, 1, 5], [1, 2, 5], [2, 3, 5], [3, 4, 5]], dtype=np.int32)     # every one has two vertices behind the eye
FLAGGED = (0, 63, 64, 69)


@functools.lru_cache(maxsize=None)
def _clip_views_fixture():
    clip = _ground_clip()
    front = clip(GROUND * [1, 1, 0.2] - [0, 0, 12])
    pos = np.stack([front] * 70)
    for k, b in enumerate(FLAGGED):
        pos[b] = clip(GROUND * [1.0 + 0.1 * k, 1, 1])
    return pos, GROUND_TRI, (24, 32)


@functools.lru_cache(maxsize=None)
def _clip_stride_fixture():
    """65 600 triangles on 8 x 8: the clip kernel's 256 workgroups of 256 lanes reach triangle 65 536 in the second trip of their
    loop.  All but four are degenerate (i, i, i) over vertices in front of the camera; the four that straddle the eye plane sit at
    0, 65 535, 65 536 and 65 599."""
    clip = _ground_clip()
    T = 65600
    pos = clip(GROUND)
    i = np.full(T, 5)                                                   # the one vertex in front
    tri = np.stack([i, i, i], axis=1).astype(np.int32)
    at = (0, 65535, 65536, 65599)
    for k, t in enumerate(at):
        tri[t] = GROUND_TRI[k]
    return pos[None], tri, (8, 8), at


def test_clip_fixtures_flag_the_views_around_64_and_pass_the_first_trip():
    pos, tri, res = _clip_views_fixture()
    behind = (pos[..., 3] <= 0).any(axis=1)
    assert tuple(np.nonzero(behind)[0]) == FLAGGED
    ids = F.ids_of(oracle_keys(pos, tri, res))
    for b in FLAGGED:
        assert (ids[b] >= 0).sum() > 100 and not np.array_equal(ids[b], ids[1]) and len(np.unique(ids[b])) >= 3
    assert (ids[1] >= 0).any() and all(np.array_equal(ids[b], ids[1]) for b in (62, 65, 68))
    pos, tri, res, at = _clip_stride_fixture()
    grid = min(256, (len(tri) + 255) // 256)
    assert grid * 256 == 65536 and at[1] < grid * 256 <= at[2] < at[3] == len(tri) - 1 and at[3] - grid * 256 < 256
    assert (pos[0, tri[list(at)], 3] <= 0).any(axis=1).all() and (pos[0, tri[list(at)], 3] > 0).any(axis=1).all()
    ids = F.ids_of(oracle_keys(pos, tri, res))
    assert set(np.unique(ids[ids >= 0]).tolist()) == set(at)              # each straddling triangle wins pixels; nothing else does


@pytest.mark.gpu
def test_clip_flagged_views_bit_exact():
    check_device(*_clip_views_fixture())


@pytest.mark.gpu
def test_clip_second_trip_bit_exact():
    pos, tri, res, _ = _clip_stride_fixture()
    check_device(pos, tri, res)
