"""Sphere initialisation (tssplat_amd/spheres_init.py): visual hull, squared distance transform, greedy cover and the multi-sphere
geometry that consumes the key points.  The device results are compared with tests/spheres_init_oracle.py bit for bit: no tolerance."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import spheres_init_oracle as O
from tssplat_amd import _capi, scenes, spheres_init

gpu = pytest.mark.gpu
INVALID = 1     # TSAMD_ERR_INVALID_ARGUMENT


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
def _edt_masks(G, seed=0):
    rng = np.random.default_rng(seed + G)
    random = rng.random((G, G, G)) < 0.5
    if random.all():
        random.flat[0] = False
    corner = np.ones((G, G, G), dtype=bool)
    corner[-1, 0, -1] = False                     # every line but one is on the sentinel after the first pass
    plane = np.ones((G, G, G), dtype=bool)
    plane[:, G // 3, :] = False
    return {"random": random, "corner": corner, "plane": plane, "all_false": np.zeros((G, G, G), dtype=bool)}


@pytest.mark.parametrize("G", [5, 17])
def test_oracle_edt_equals_scipy(G):
    ndimage = pytest.importorskip("scipy.ndimage")
    for name, mask in _edt_masks(G).items():
        want = np.rint(ndimage.distance_transform_edt(mask) ** 2).astype(np.int32)
        got = O.distance_transform_sq(mask)
        assert got.dtype == np.int32 and np.array_equal(got, want), name
    with pytest.raises(ValueError):
        O.distance_transform_sq(np.ones((G, G, G), dtype=bool))


def test_key_points_json_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    kp = spheres_init.KeyPoints(rng.standard_normal((5, 3)).astype(np.float32), rng.random(5).astype(np.float32), 0.25, 0.5)
    path = tmp_path / "mario.json"
    kp.save_json(path)
    raw = json.load(open(path))
    assert set(raw) == {"pt", "r"}                                        # generate_init_spheres.py:536-539
    assert len(raw["pt"]) == 5 and all(len(p) == 3 for p in raw["pt"])
    assert len(raw["r"]) == 5 and all(isinstance(r, list) and len(r) == 1 for r in raw["r"])   # radius.tolist() of an [S, 1] array
    # ... which is what the reference's consumer reads (tetmesh_geometry.py:235-239)
    assert np.asarray(raw["pt"]).shape == (5, 3) and np.asarray(raw["r"]).shape == (5, 1)
    back = spheres_init.KeyPoints.load_json(path)
    assert back.pt.dtype == np.float32 and back.r.dtype == np.float32
    assert back.pt.tobytes() == kp.pt.tobytes() and back.r.tobytes() == kp.r.tobytes()
    assert back.hull_fraction is None and back.uncovered_fraction is None
    flat = tmp_path / "flat.json"                                         # radii as plain numbers load too
    json.dump({"pt": kp.pt.tolist(), "r": kp.r.tolist()}, open(flat, "w"))
    assert spheres_init.KeyPoints.load_json(flat).r.tobytes() == kp.r.tobytes()
    empty = spheres_init.KeyPoints(np.zeros((0, 3)), np.zeros(0))
    empty.save_json(path)
    back = spheres_init.KeyPoints.load_json(path)
    assert back.pt.shape == (0, 3) and back.r.shape == (0,)
    with pytest.raises(ValueError):
        spheres_init.KeyPoints(np.zeros((2, 3)), np.zeros(3))


def test_c_abi_argument_errors_launch_nothing():
    """Every argument error is reported before anything touches the device: all device pointers here are null or made up."""
    lib = _capi.load()
    p = 0x1000                                                            # "not null"; never dereferenced on these paths

    def carve(alpha=p, batch=2, height=8, width=8, channels=2, channel=1, mvp=p, grid=8, lo=-1.0, hi=1.0, bits=p, hull=p):
        return lib.tsamd_hull_carve(alpha, batch, height, width, channels, channel, 0.5, mvp, grid, lo, hi, bits, hull, None)

    def edt(mask=p, grid=8, ws=p, d2=p, status=p):
        return lib.tsamd_edt_squared(mask, grid, ws, d2, status, None)

    def cover(hull=p, d2=p, grid=8, n=4, s2=1.0, hs2=1.0, m2=0.0, ws=p, unc=p, flat=p, q=p, count=p):
        return lib.tsamd_greedy_cover(hull, d2, grid, n, s2, hs2, m2, ws, unc, flat, q, count, None)

    cases = [
        (carve, dict(grid=0), "grid"), (carve, dict(grid=513), "grid"), (carve, dict(grid=-3), "grid"),
        (carve, dict(batch=-1), "batch"), (carve, dict(height=-1), "height"), (carve, dict(width=-1), "width"), (carve, dict(width=8193), "width"),
        (carve, dict(height=0), "height"), (carve, dict(channels=-1), "channels"), (carve, dict(channel=2), "channel"), (carve, dict(channel=-1), "channel"),
        (carve, dict(channels=0, channel=0), "channel"), (carve, dict(lo=1.0, hi=1.0), "lo"), (carve, dict(hi=float("nan")), "lo"),
        (carve, dict(alpha=None), "alpha_dev"), (carve, dict(mvp=None), "mvp_dev"), (carve, dict(bits=None), "bits_workspace_dev"),
        (carve, dict(hull=None), "hull_out_dev"), (carve, dict(batch=0, alpha=None, mvp=None, bits=None, hull=None), "hull_out_dev"),
        (edt, dict(grid=0), "grid"), (edt, dict(grid=513), "grid"), (edt, dict(mask=None), "mask_dev"), (edt, dict(ws=None), "workspace_dev"),
        (edt, dict(d2=None), "d2_out_dev"), (edt, dict(status=None), "status_out_dev"),
        (cover, dict(grid=0), "grid"), (cover, dict(grid=513), "grid"), (cover, dict(n=-1), "n_spheres"), (cover, dict(n=(1 << 20) + 1), "n_spheres"),
        (cover, dict(s2=-1.0), "s2"), (cover, dict(hs2=float("nan")), "s2"), (cover, dict(hull=None), "hull_dev"), (cover, dict(d2=None), "d2_dev"),
        (cover, dict(ws=None), "workspace_dev"), (cover, dict(unc=None), "uncovered_out_dev"), (cover, dict(count=None), "count_out_dev"),
        (cover, dict(flat=None), "flat_out_dev"), (cover, dict(q=None), "q_out_dev"),
    ]
    for fn, kw, word in cases:
        assert fn(**kw) == INVALID, (fn.__name__, kw)
        msg = lib.tsamd_last_error().decode()
        assert msg and word in msg, (fn.__name__, kw, msg)


def test_python_arguments_are_checked_by_name():
    """Nothing here reaches the library: a CPU tensor is refused first, with the argument's name."""
    a, m = torch.zeros(1, 4, 4, 1), torch.zeros(1, 4, 4)
    for call, word in [(lambda: spheres_init.visual_hull(a, m), "alpha"), (lambda: spheres_init.visual_hull(a, m, grid=0), "grid"),
                       (lambda: spheres_init.visual_hull(a, m, bounds=(1.0, 1.0)), "bounds"),
                       (lambda: spheres_init.distance_transform_sq(torch.zeros(2, 2, 2, dtype=torch.bool)), "mask"),
                       (lambda: spheres_init.greedy_cover(torch.zeros(2, 2, 2, dtype=torch.bool), torch.zeros(2, 2, 2, dtype=torch.int32), 1), "hull"),
                       (lambda: spheres_init.init_spheres(a, m, -1), "n_spheres"), (lambda: spheres_init.init_spheres(a, m, 2, shrink=0.0), "shrink")]:
        with pytest.raises(RuntimeError, match=word):
            call()


# ---------------------------------------------------------------- hull ----------------------------------------------------------------
THRESHOLD = 0.5


@functools.lru_cache(maxsize=None)
def _hull_scene(B, H, W):
    """alpha [B, H, W, 2] (channel 1 is the silhouette: big blobs in steps of 1/8, so many pixels sit exactly on the threshold; one
    NaN pixel; channel 0 is noise) and the cameras: B = 1 the view scaled past |ndc| = 1, B = 3 an orbit view, the scaled view and
    a view from inside the cube."""
    rng = np.random.default_rng(100 * B + H)
    orbit = scenes.orbit_mvps(3)
    scaled = orbit[1].copy()
    scaled[:2] *= 1.9                                                     # part of the cube projects outside |ndc| < 1
    within = scenes.orbit_mvps(1, distance=0.6, near=0.05)[0]             # eye inside [-1, 1]^3: voxels behind it have w <= 0
    mvp = np.stack([scaled] if B == 1 else [orbit[0], scaled, within]).astype(np.float32)
    yy, xx = np.meshgrid((np.arange(H) + 0.5) / H, (np.arange(W) + 0.5) / W, indexing="ij")
    alpha = rng.random((B, H, W, 2)).astype(np.float32)
    for b in range(B):
        blob = np.zeros((H, W))
        for _ in range(3):
            cy, cx, rad = rng.uniform(0.3, 0.7), rng.uniform(0.3, 0.7), rng.uniform(0.35, 0.6)
            blob = np.maximum(blob, 1.25 - np.hypot(yy - cy, xx - cx) / rad)
        alpha[b, :, :, 1] = np.round(np.clip(blob, 0, 1) * 8) / 8
    assert (alpha[..., 1] == THRESHOLD).sum() >= B                        # pixels exactly on the threshold: strict > leaves them out
    on = np.argwhere(alpha[0, :, :, 1] > THRESHOLD)
    y, x = on[len(on) // 2]
    alpha[0, y, x, 1] = np.nan
    return alpha, mvp


@gpu
@pytest.mark.parametrize("HW", [(24, 40), (31, 33)])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("G", [5, 33])
def test_visual_hull_equals_oracle(G, B, HW):
    alpha, mvp = _hull_scene(B, *HW)
    want = O.visual_hull(alpha, mvp, G, (-1.0, 1.0), THRESHOLD, 1)
    # the scene exercises what it is meant to: float64 clip coordinates of the voxel centres
    c = O.voxel_centres(G).astype(np.float64)
    P = np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3)
    clip = np.einsum("brc,nc->bnr", mvp.astype(np.float64), np.concatenate([P, np.ones((P.shape[0], 1))], 1))
    if B == 3:
        assert (clip[2, :, 3] <= 0).any() and (clip[2, :, 3] > 0).any()
    front = clip[-2 if B == 3 else 0]
    assert (np.abs(front[:, 0] / front[:, 3]) >= 1).any()
    if G == 33:
        assert 0 < want.sum() < want.size
    got = spheres_init.visual_hull(dev(alpha), dev(mvp), grid=G, threshold=THRESHOLD, channel=1)
    assert got.dtype == torch.bool and tuple(got.shape) == (G, G, G)
    assert np.array_equal(got.cpu().numpy(), want), (int(got.sum()), int(want.sum()))
    if G == 33 and B == 3:      # the other channel is another silhouette: the channel argument selects
        other = spheres_init.visual_hull(dev(alpha), dev(mvp), grid=G, threshold=THRESHOLD, channel=0)
        assert np.array_equal(other.cpu().numpy(), O.visual_hull(alpha, mvp, G, (-1.0, 1.0), THRESHOLD, 0))


# The pack kernel writes two 32-bit words per 64 pixels, the second one only when the row has it.  Under the identity matrix clip_w = 1 and
# ndc = (x, y) of the voxel centre, so with G >= max(H, W) every pixel decides some voxel and a wrong bit anywhere shows in the hull.
PACK_HEIGHT = 5
PACK_WIDTHS = [1, 31, 32, 33, 63, 64, 65, 96, 97, 128, 129]


def _pack_grid(W):
    return 33 if W <= 33 else min(G for G in (65, 129) if G >= W)


@functools.lru_cache(maxsize=None)
def _pack_scene(W):
    """alpha [2, PACK_HEIGHT, W, 2]: random values around the threshold in both channels and both images, three pixels of channel 1 exactly
    on it, one NaN and one pixel that is on in both images; two identity matrices."""
    rng = np.random.default_rng(1000 + W)
    alpha = (THRESHOLD + rng.uniform(-0.25, 0.4, (2, PACK_HEIGHT, W, 2))).astype(np.float32)
    for n in range(3):
        alpha[n % 2, (2 * n + 1) % PACK_HEIGHT, (7 * n + W // 2) % W, 1] = THRESHOLD
    alpha[1, 2, W - 1, 1] = np.nan
    alpha[:, 4, W - 1] = (0.125, 0.875)                                   # the row's last pixel: on in both images of channel 1, off in channel 0
    return alpha, np.stack([np.eye(4, dtype=np.float32)] * 2)


@functools.lru_cache(maxsize=None)
def _pack_want(W):
    alpha, mvp = _pack_scene(W)
    return O.visual_hull(alpha, mvp, _pack_grid(W), (-1.0, 1.0), THRESHOLD, 1)


def _pack_preconditions(W):
    """Every pixel is the pixel of some voxel centre, and the pixels of the row's last word decide voxels of the hull."""
    alpha, mvp = _pack_scene(W)
    G, H = _pack_grid(W), PACK_HEIGHT
    c = O.voxel_centres(G)
    one, half = np.float32(1.0), np.float32(0.5)
    px = np.minimum(W - 1, np.floor(((c + one) * half) * np.float32(W)).astype(np.int64))      # the oracle's pixel of ndc = c, c1 = c / 1
    py = np.minimum(H - 1, np.floor(((c + one) * half) * np.float32(H)).astype(np.int64))
    assert (np.abs(c) < 1).all() and set(px.tolist()) == set(range(W)) and set(py.tolist()) == set(range(H)) and G >= max(H, W)
    assert (alpha[..., 1] == THRESHOLD).sum() == 3 and np.isnan(alpha[..., 1]).sum() == 1
    words = (W + 31) // 32
    cleared = alpha.copy()
    cleared[:, :, 32 * (words - 1):, 1] = 0.0
    want = _pack_want(W)
    assert 0 < want.sum() < want.size
    assert (O.visual_hull(cleared, mvp, G, (-1.0, 1.0), THRESHOLD, 1) != want).any()
    assert (O.visual_hull(alpha, mvp, G, (-1.0, 1.0), THRESHOLD, 0) != want).any()             # the channel matters too


@pytest.mark.parametrize("W", PACK_WIDTHS)
def test_edge_pack_widths_are_reached(W):
    _pack_preconditions(W)


@gpu
@pytest.mark.parametrize("W", PACK_WIDTHS)
def test_edge_pack_widths(W):
    """W <= 32: one word, the second must not be written.  65: two chunks, three words.  129: three chunks, five words."""
    alpha, mvp = _pack_scene(W)
    G, want = _pack_grid(W), _pack_want(W)
    assert 0 < want.sum() < want.size
    got = spheres_init.visual_hull(dev(alpha), dev(mvp), grid=G, threshold=THRESHOLD, channel=1)
    assert got.dtype == torch.bool and tuple(got.shape) == (G, G, G)
    assert np.array_equal(got.cpu().numpy(), want), (int(got.sum()), int(want.sum()))


# ---------------------------------------------------------------- EDT ----------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", ["random", "corner", "plane", "all_false"])
@pytest.mark.parametrize("G", [1, 5, 33, 65])
def test_distance_transform_equals_oracle(G, kind):
    mask = _edt_masks(G)[kind]
    got = spheres_init.distance_transform_sq(dev(mask))
    assert got.dtype == torch.int32 and tuple(got.shape) == (G, G, G)
    want = O.distance_transform_sq(mask)
    if kind == "all_false":
        assert not want.any()
    assert np.array_equal(got.cpu().numpy(), want)


@gpu
@pytest.mark.parametrize("G", [1, 5, 33, 65])
def test_distance_transform_of_a_full_mask_is_an_error(G):
    with pytest.raises(ValueError, match="no false voxel"):
        spheres_init.distance_transform_sq(torch.ones((G, G, G), dtype=torch.bool, device="cuda"))


# ---------------------------------------------------------------- greedy cover ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _two_balls(G=24):
    """Two equal balls, mirror images in the first axis, and the oracle's transform of them."""
    i, j, k = np.meshgrid(*(np.arange(G),) * 3, indexing="ij")
    hull = np.zeros((G, G, G), dtype=bool)
    for ci in (6, G - 1 - 6):
        hull |= (i - ci) ** 2 + (j - 12) ** 2 + (k - 11) ** 2 <= 25
    return hull, O.distance_transform_sq(hull)


def _cover_both(hull, d2, n, **kw):
    flat, q, unc = spheres_init.greedy_cover(dev(hull), dev(d2), n, **kw)
    wf, wq, wu = O.greedy_cover(hull, d2, n, **kw)
    assert flat.dtype == torch.int64 and q.dtype == torch.int32 and unc.dtype == torch.bool
    assert tuple(flat.shape) == tuple(q.shape) == (len(wf),) and tuple(unc.shape) == hull.shape
    assert np.array_equal(flat.cpu().numpy(), wf) and np.array_equal(q.cpu().numpy(), wq) and np.array_equal(unc.cpu().numpy(), wu)
    return wf, wq, wu


@gpu
def test_greedy_cover_tie_goes_to_the_lower_index():
    hull, d2 = _two_balls()
    flat, q, _ = _cover_both(hull, d2, 2)
    assert len(flat) == 2 and q[0] == q[1] and flat[0] < flat[1]
    assert d2.reshape(-1)[flat[0]] == d2.max() and (d2 == d2.max()).sum() >= 2


@gpu
def test_greedy_cover_stops_at_min_radius():
    hull, d2 = _two_balls()
    flat, q, unc = _cover_both(hull, d2, 64, min_radius=0.15)
    assert 2 <= len(flat) < 64 and unc.any()                              # balls below min_radius are never placed
    h = 2.0 / hull.shape[0]
    assert (np.sqrt(q.astype(np.float64)) * h * 0.92 >= 0.15 - 1e-12).all()


@gpu
def test_greedy_cover_of_nothing():
    hull, d2 = _two_balls()
    flat, q, unc = _cover_both(hull, d2, 0)
    assert len(flat) == 0 and np.array_equal(unc, hull)
    empty = np.zeros_like(hull)
    flat, q, unc = _cover_both(empty, np.zeros(hull.shape, dtype=np.int32), 5)
    assert len(flat) == 0 and not unc.any()


@gpu
def test_greedy_cover_without_shrink_and_repeatable():
    hull, d2 = _two_balls()
    _cover_both(hull, d2, 12, shrink=1.0, min_radius=0.01)                # covered iff D2 <= q: an equality on integers
    a = spheres_init.greedy_cover(dev(hull), dev(d2), 12, min_radius=0.01)
    b = spheres_init.greedy_cover(dev(hull), dev(d2), 12, min_radius=0.01)
    for x, y in zip(a, b):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


# greedy_cover_kernel strides over kCoverBlocks * 256 voxels; at G = 96 the volume takes two trips.
COVER_STRIDE = 2048 * 256
STRIDE_GRID = 96


@functools.lru_cache(maxsize=None)
def _stride_balls():
    """_two_balls at G = 96: the balls of radius 10 around i = 20 and i = 75 lie on either side of flat index COVER_STRIDE."""
    G = STRIDE_GRID
    i, j, k = np.meshgrid(*(np.arange(G),) * 3, indexing="ij")
    hull = np.zeros((G, G, G), dtype=bool)
    for ci in (20, G - 1 - 20):
        hull |= (i - ci) ** 2 + (j - 48) ** 2 + (k - 47) ** 2 <= 100
    return hull, O.distance_transform_sq(hull)


def _upper_ball():
    """Only the ball whose voxels all lie at or past COVER_STRIDE (d2 inside it is unchanged: the other ball is far away)."""
    hull, d2 = _stride_balls()
    upper = hull.copy()
    upper[:STRIDE_GRID // 2] = False
    return upper, np.where(upper, d2, 0).astype(np.int32)


STRIDE_RUNS = {"defaults": dict(n=2), "min_radius": dict(n=64, min_radius=0.027), "no_shrink": dict(n=12, shrink=1.0, min_radius=0.02)}


@functools.lru_cache(maxsize=None)
def _stride_want(run, upper=False):
    kw = dict(STRIDE_RUNS[run])
    return O.greedy_cover(*(_upper_ball() if upper else _stride_balls()), kw.pop("n"), **kw)


def _stride_preconditions():
    hull, d2 = _stride_balls()
    assert hull.size > COVER_STRIDE and hull.size <= 2 * COVER_STRIDE
    top = np.nonzero(d2.reshape(-1) == d2.max())[0]
    assert top.tolist() == [(20 * 96 + 48) * 96 + 47, (75 * 96 + 48) * 96 + 47] and top[0] < COVER_STRIDE <= top[1]       # the two maxima tie
    flat, q, _ = _stride_want("defaults")
    assert flat.tolist() == top.tolist() and q[0] == q[1] == d2.max()                          # ... and the lower index goes first
    flat, q, unc = _stride_want("min_radius")
    assert 2 < len(flat) < STRIDE_RUNS["min_radius"]["n"] and unc.any() and (flat < COVER_STRIDE).any() and (flat >= COVER_STRIDE).any()
    flat, q, unc = _stride_want("no_shrink")
    assert len(flat) >= 2
    upper, _ = _upper_ball()
    assert upper.any() and np.nonzero(upper.reshape(-1))[0].min() >= COVER_STRIDE
    flat, q, unc = _stride_want("min_radius", True)
    assert len(flat) > 1 and (flat >= COVER_STRIDE).all()


def test_edge_cover_stride_is_reached():
    _stride_preconditions()


@gpu
@pytest.mark.parametrize("run", sorted(STRIDE_RUNS))
def test_edge_cover_stride(run):
    hull, d2 = _stride_balls()
    top = np.nonzero(d2.reshape(-1) == d2.max())[0]
    assert len(top) == 2 and top[0] < COVER_STRIDE <= top[1]
    kw = dict(STRIDE_RUNS[run])
    n = kw.pop("n")
    flat, q, unc = spheres_init.greedy_cover(dev(hull), dev(d2), n, **kw)
    wf, wq, wu = _stride_want(run)
    assert flat.dtype == torch.int64 and q.dtype == torch.int32 and unc.dtype == torch.bool
    assert np.array_equal(flat.cpu().numpy(), wf) and np.array_equal(q.cpu().numpy(), wq) and np.array_equal(unc.cpu().numpy(), wu)
    assert len(wf) >= 2 and wf[0] == top[0] and wf[1] == top[1]


@gpu
def test_edge_cover_finds_what_lies_past_the_first_stride():
    hull, d2 = _upper_ball()
    assert np.nonzero(hull.reshape(-1))[0].min() >= COVER_STRIDE
    kw = dict(STRIDE_RUNS["min_radius"])
    flat, q, unc = spheres_init.greedy_cover(dev(hull), dev(d2), kw.pop("n"), **kw)
    wf, wq, wu = _stride_want("min_radius", True)
    assert len(wf) > 1 and np.array_equal(flat.cpu().numpy(), wf) and np.array_equal(q.cpu().numpy(), wq) and np.array_equal(unc.cpu().numpy(), wu)


# ---------------------------------------------------------------- end to end ----------------------------------------------------------------
@gpu
def test_init_spheres_end_to_end(tmp_path):
    import tssplat_amd.dr as dr
    from tssplat_amd import geometry
    G, n_spheres, res, views = 24, 6, 64, 8
    bv, bt = scenes.kuhn_ball(3)
    bv = bv / np.linalg.norm(bv, axis=1).max()
    vid, faces = geometry.get_surface_vf(bt)
    sv = bv[vid]
    verts = np.concatenate([sv * 0.36 + [-0.47, 0.05, 0.0], sv * 0.3 + [0.45, -0.1, 0.1]]).astype(np.float32)
    tri = np.concatenate([faces, faces + sv.shape[0]]).astype(np.int32)
    mvp = dev(scenes.orbit_mvps(views))
    posw = torch.cat([dev(verts), torch.ones(verts.shape[0], 1, device="cuda")], dim=1)
    pos_clip = torch.matmul(posw, mvp.transpose(1, 2)).contiguous()
    rast, _ = dr.rasterize(dr.RasterizeCudaContext(), pos_clip, dev(tri), resolution=[res, res], grad_db=False)
    alpha = torch.clamp(rast[..., -1:], 0, 1).contiguous()

    kp = spheres_init.init_spheres(alpha, mvp, n_spheres=n_spheres, grid=G)
    want = O.init_spheres(alpha.cpu().numpy(), mvp.cpu().numpy(), n_spheres, G)
    S = len(kp)
    assert 2 <= S <= n_spheres and S == len(want["r"])
    assert kp.pt.tobytes() == want["pt"].tobytes() and kp.r.tobytes() == want["r"].tobytes()
    assert kp.hull_fraction == want["hull_fraction"] and kp.uncovered_fraction == want["uncovered_fraction"]
    assert 0 < kp.hull_fraction < 1 and 0 <= kp.uncovered_fraction < 1
    hull, flat, q = want["hull"], want["flat"], want["q"].astype(np.int64)
    assert hull.reshape(-1)[flat].all()                                   # every centre lies in the hull
    assert (np.diff(kp.r) <= 0).all() and (kp.r.astype(np.float64) ** 2 >= 0.05 ** 2).all()
    ijk = np.stack(np.unravel_index(flat, hull.shape), 1)
    for a in range(S):
        for b in range(a + 1, S):                                         # a later centre is not inside an earlier ball
            assert not float(((ijk[a] - ijk[b]) ** 2).sum()) <= float(q[a]) * (0.92 * 0.92)
    assert np.array_equal(kp.pt, O.voxel_centres(G)[ijk])

    geo = geometry.TetMeshMultiSphereGeometry(kp, k=2)
    tv, tt = scenes.kuhn_ball(2)
    tv = tv / np.linalg.norm(tv, axis=1).max()
    n = tv.shape[0]
    assert tuple(geo.tet_v.shape) == (S * n, 3) and tuple(geo.tet_elem.shape) == (S * tt.shape[0], 4)
    assert sorted(v for idx in geo.all_spheres_vtx_idx for v in idx) == list(range(S * n)) and len(geo.all_spheres_vtx_idx) == S
    assert all(np.array_equal(e, tt) for e in geo.all_spheres_elem_idx) and len(geo.all_spheres_elem_idx) == S
    energy = geo(0).smooth_barrier_energy
    assert torch.isfinite(energy).all()
    rest = np.concatenate([(tv * float(r) + c.astype(np.float64)).astype(np.float32) for c, r in zip(kp.pt, kp.r)])
    elem = np.concatenate([tt + s * n for s in range(S)]).astype(np.int32)
    assert np.array_equal(geo.tet_v.detach().cpu().numpy(), rest) and np.array_equal(geo.tet_elem.cpu().numpy(), elem)
    param = {"smooth_eng_coeff": 2e-4, "barrier_coeff": 2e-4, "increase_order_iter": 1000}
    plain = geometry.TetMeshGeometry(rest, elem, smooth_barrier_param=dict(param, smooth_eng_coeff=param["smooth_eng_coeff"] / S))
    assert plain(0).smooth_barrier_energy.detach().cpu().numpy().tobytes() == energy.detach().cpu().numpy().tobytes()
    # the caller's parameters are copied, not divided in place; a key-point file gives the same geometry
    geo2 = geometry.TetMeshMultiSphereGeometry(kp, k=2, smooth_barrier_param=param)
    assert param["smooth_eng_coeff"] == 2e-4
    assert geo2(0).smooth_barrier_energy.detach().cpu().numpy().tobytes() == energy.detach().cpu().numpy().tobytes()
    kp.save_json(tmp_path / "kp.json")
    geo3 = geometry.TetMeshMultiSphereGeometry(str(tmp_path / "kp.json"), template=(tv, tt), use_smooth_barrier=False)
    assert np.array_equal(geo3.tet_v.detach().cpu().numpy(), rest)

    out = tmp_path / "export"
    geo.export(str(out), "final")
    names = {"final.veg", "final_vtx.npy", "final_elem.npy"} | {f"final_sp{i}_{w}.npy" for i in range(S) for w in ("vtx", "elem")}
    assert set(os.listdir(out)) == names
    assert np.array_equal(np.load(out / "final_vtx.npy"), rest) and np.array_equal(np.load(out / "final_elem.npy"), elem)
    tet_v = geo.tet_v.detach().cpu().numpy()
    for i in range(S):
        assert np.array_equal(np.load(out / f"final_sp{i}_vtx.npy"), tet_v[geo.all_spheres_vtx_idx[i]])
        assert np.array_equal(np.load(out / f"final_sp{i}_elem.npy"), tt)
    v, t = scenes.read_veg(out / "final.veg")
    assert np.array_equal(v.astype(np.float32), rest) and np.array_equal(t, elem)
