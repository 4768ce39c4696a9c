"""The colour stage under a blend plan: dr.plan_blends, dr.shade, dr.shade_l1, the seven tsamd_shade* entry points and the opt-in
callers in MeshRasterizer, against the float64 oracle (tests/shade_oracle.py over oracle/raster_oracle.py) and against the
operators path (scatter -> lerp -> antialias -> L1Loss) on the same GPU.

CPU tier: what the kernels rely on -- under a fixed ``rast`` the antialias blends are data, and the image and its gradient are
the two groupings of those records -- asserted on the oracle alone, and the argument checks of the C ABI.  GPU tier: every case
asserts on the GPU's own ``rast`` what its scene is there for before it looks at a kernel's output.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import aa_scenes as S
import shade_oracle as O
from oracle import raster_oracle as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UPSTREAM = 3.0          # d objective / d loss of the gradient cases (not 1)


def _scene_condition(scene, rast, pos, tri, events, dst, src):
    """What the scene is there for, on the ``rast`` the caller is about to use."""
    B, H, W = rast.shape[:3]
    cov = (rast[..., 3] > 0).reshape(-1)
    per_view = cov.reshape(B, -1).sum(axis=1)
    both = int((cov[dst] & cov[src]).sum()) if len(dst) else 0
    if scene == "checker_and_sheet":
        assert (H * W) % 64 != 0 and all(len(e) > 100 for e in events)
        flat = S.differing_pairs(rast).reshape(-1, 2).any(axis=1)
        for b in range(1, B):                                      # the chunk that straddles views b - 1 | b: pairs on both sides
            k = b * H * W // 64
            assert flat[64 * k:b * H * W].any() and flat[b * H * W:64 * (k + 1)].any()
        slots = S.edge_slots(tri)
        assert sum(len(slots[(min(ev[5]), max(ev[5]))]) == 1 for evs in events for ev in evs) >= 100      # open borders: no partner
    elif scene == "sparse_checker":
        assert (S.pairs_per_chunk(rast) == 128).sum() >= 8
        assert 2 <= O.most_per_group(dst) <= 4 and O.most_per_group(src) >= 2
    elif scene == "soup":
        assert both >= 100                                         # foreground / foreground pairs, decided by depth
    elif scene == "backdrop_and_sheet":
        assert cov.all() and both == len(dst) >= 50
    elif scene == "empty_and_covered":
        assert per_view[0] > 100 and per_view[1] == 0 and len(events[0]) > 50 and len(events[1]) == 0
    elif scene == "nothing_covered":
        assert not cov.any() and len(dst) == 0
    assert O.most_per_group(dst) <= 4


def _ambiguous(out64, target, K):
    """Elements whose sign the float32 image cannot be held to: |out64 - t64| inside the image bound."""
    return np.abs(out64[..., :3] - np.asarray(target, dtype=np.float32).astype(np.float64)[..., :3]) <= O.image_bound(K)


def _excluded_gradient_entries(amb, rast, dst, src):
    """``[N, 3]`` bool: a grad_color entry reads an ambiguous sign -- its own pixel's or a destination's it feeds."""
    pp, _ = O.pix_point(rast)
    amb = amb.reshape(-1, 3)
    hit = amb.copy()
    np.logical_or.at(hit, src, amb[dst])
    return hit[pp >= 0]


# ================================================================ CPU tier ================================================================

@functools.lru_cache(maxsize=None)
def _cpu_case(scene):
    build, res = O.SCENES[scene]
    pos, tri = build()
    rast = R.rasterize(pos, tri, res)
    events = R.antialias_events(rast, pos, tri)
    dst, src, wgt = O.records(events, *res)
    _, n_points = O.pix_point(rast)
    return pos, tri, rast, events, dst, src, wgt, n_points, O.inputs(scene, n_points, rast.shape[:3])


@pytest.mark.parametrize("scene", sorted(O.SCENES))
def test_the_plan_formulation_is_the_operators_path_on_the_oracle(scene):
    """Image: per destination its records in order on ``c_p`` from ``pix_point`` == ``R.antialias(lerp(bg, scatter(color), mask))``,
    bit for bit.  Gradient: the transposed form == ``R.antialias_backward`` gathered at the foreground (other summation order:
    1e-12 of the upstream scale).  The share of elements whose sign is discrete within the image bound is <= 0.1 % for the seeds
    the GPU tier uses."""
    pos, tri, rast, events, dst, src, wgt, n_points, (color, background, target) = _cpu_case(scene)
    _scene_condition(scene, rast, pos, tri, events, dst, src)
    want = O.shade_operators(color, background, rast, pos, tri, events)
    got = O.shade_csr(color, background, rast, dst, src, wgt)
    assert want.shape == rast.shape[:3] + (3,) and np.array_equal(got, want)
    if len(dst):
        assert (np.abs(want - O.composite(color, background, rast)) > 0).sum() >= len(np.unique(dst))
    g = O.l1_grad(want, target, UPSTREAM)
    G = UPSTREAM / want.size
    a = O.grad_color_csr(g, rast, dst, src, wgt)
    b = O.grad_color_operators(g, color, background, rast, pos, tri, events)
    assert a.shape == (n_points, 3) and np.all(np.abs(a - b) <= 1e-12 * G)
    K = O.most_per_group(dst)
    amb = _ambiguous(want, target, K)
    assert amb.mean() <= 1e-3
    if n_points:
        assert _excluded_gradient_entries(amb, rast, dst, src).mean() <= 1e-3 and np.abs(a).max() > 0


@pytest.mark.parametrize("scene", ["checker_and_sheet", "soup"])
def test_the_transposed_gradient_is_the_derivative_of_the_oracle_loss(scene):
    """Central differences of ``UPSTREAM * l1(shade(color))`` in float64 at points whose own pixel and destinations are further than
    2e-3 from ``out = t`` (L1 is piecewise linear: the difference quotient is exact there up to rounding)."""
    pos, tri, rast, events, dst, src, wgt, n_points, (color, background, target) = _cpu_case(scene)
    out = O.shade_csr(color, background, rast, dst, src, wgt)
    grad = O.grad_color_csr(O.l1_grad(out, target, UPSTREAM), rast, dst, src, wgt)
    pp, _ = O.pix_point(rast)
    near = (np.abs(out - target.astype(np.float64)[..., :3]) <= 2e-3).reshape(-1, 3)
    unsafe = near.copy()
    np.logical_or.at(unsafe, src, near[dst])
    unsafe = unsafe[pp >= 0]
    point_of_pixel = pp
    sources = np.unique(point_of_pixel[src][point_of_pixel[src] >= 0])              # points that feed a destination
    rng = np.random.default_rng(2)
    picks = [(int(k), int(c)) for k in rng.choice(sources, 12, replace=False) for c in range(3) if not unsafe[k, c]]
    picks += [(int(k), 1) for k in rng.choice(n_points, 6, replace=False) if not unsafe[k, 1]]
    assert len(picks) >= 30
    h = 1e-3
    col = color.astype(np.float64)
    for k, c in picks:
        vals = []
        for sgn in (1.0, -1.0):
            moved = col.copy()
            moved[k, c] += sgn * h
            # (float64 colours: R-free formulation, the float32 casts inside shade_csr would round the step)
            bgd = background.astype(np.float64).reshape(-1, 3)
            cc = np.where((pp >= 0)[:, None], moved[np.maximum(pp, 0)], bgd)
            o = cc.copy()
            np.add.at(o, dst, wgt[:, None] * (cc[src] - cc[dst]))
            vals.append(UPSTREAM * np.mean(np.abs(o.reshape(out.shape) - target.astype(np.float64)[..., :3])))
        fd = (vals[0] - vals[1]) / (2 * h)
        assert abs(fd - grad[k, c]) <= 1e-6 * UPSTREAM / out.size, (k, c, fd, grad[k, c])      # (entries are multiples of G = UPSTREAM / n)


def test_shade_abi_rejects_bad_arguments():
    """The seven entry points check their arguments before any device call (this test runs without a GPU) and name what is wrong;
    tsamd_shade_l1_workspace_bytes is monotone and 256-byte aligned."""
    from tssplat_amd import _capi
    lib = _capi.load()
    p = ctypes.c_void_p(256)                                       # a non-null pointer that is never dereferenced: every call below fails first

    def err(rc):
        assert rc != 0
        return lib.tsamd_last_error().decode()

    def plan(**kw):
        st = _capi.BlendPlanStruct()
        st.struct_size = ctypes.sizeof(_capi.BlendPlanStruct)
        st.batch, st.height, st.width, st.n_points, st.n_blends, st.n_dst, st.n_src = 1, 8, 8, 10, 6, 4, 5
        for name, _ in _capi.BlendPlanStruct._fields_:
            if name.endswith("_dev"):
                setattr(st, name, 256)
        for k, v in kw.items():
            setattr(st, k, v)
        return ctypes.byref(st)

    calls = {
        "shade": lambda pl, a=p, b=p, c=p: lib.tsamd_shade(pl, a, b, c, None),
        "shade_backward": lambda pl, a=p, b=p: lib.tsamd_shade_backward(pl, a, b, None),
        "shade_l1": lambda pl, a=p, b=p, c=p, ch=3, ws=p, loss=p: lib.tsamd_shade_l1(pl, a, b, c, ch, ws, loss, None, None, None, None),
        "shade_l1_backward": lambda pl, a=p, b=p, c=p, d=p: lib.tsamd_shade_l1_backward(pl, a, b, c, d, None),
    }
    for name, call in calls.items():
        assert err(call(None)).endswith("plan is null"), name
        assert "struct_size" in err(call(plan(struct_size=8))), name
        for kw in ({"height": 8193}, {"width": -1}, {"batch": -1}):
            assert "out of range (0 .. 8192 pixels per side)" in err(call(plan(**kw))), (name, kw)
        assert "below 2^30 pixels" in err(call(plan(batch=1 << 20, height=64, width=64))), name
        assert "n_points out of range" in err(call(plan(n_points=65))), name
        assert "n_points out of range" in err(call(plan(n_points=-1))), name
        assert "n_blends out of range" in err(call(plan(n_blends=-1))), name
        assert "at most 2^31 - 1" in err(call(plan(batch=1 << 14, height=200, width=200, n_blends=1 << 31))), name
        assert "n_dst / n_src out of range" in err(call(plan(n_dst=7))), name
        assert "n_dst / n_src out of range" in err(call(plan(n_src=-1))), name
        for field in ("pix_point_dev", "pix_dst_dev", "dst_ptr_dev", "dst_src_pix_dev", "dst_src_point_dev", "dst_weight_dev", "src_ptr_dev",
                      "src_dst_pix_dev", "src_dst_slot_dev", "src_weight_dev", "point_pix_dev", "point_dst_dev", "point_src_dev"):
            assert err(call(plan(**{field: None}))).endswith(f"plan->{field} is null"), (name, field)
    assert err(calls["shade"](plan(), a=None)).endswith("color_dev is null")
    assert err(calls["shade"](plan(), b=None)).endswith("background_dev is null")
    assert err(calls["shade"](plan(), c=None)).endswith("out_dev is null")
    assert err(calls["shade_backward"](plan(), a=None)).endswith("grad_out_dev is null")
    assert err(calls["shade_backward"](plan(), b=None)).endswith("grad_color_dev is null")
    for kw, word in (({"a": None}, "color_dev"), ({"b": None}, "background_dev"), ({"c": None}, "target_dev"), ({"ws": None}, "workspace_dev"),
                     ({"loss": None}, "loss_out_dev")):
        assert err(calls["shade_l1"](plan(), **kw)).endswith(word + " is null"), kw
    for ch in (0, 1, 2, 5):
        assert "target_channels must be 3 or 4" in err(calls["shade_l1"](plan(), ch=ch))
    assert "go together" in err(lib.tsamd_shade_l1(plan(), p, p, p, 4, p, p, None, p, None, None))
    assert "go together" in err(lib.tsamd_shade_l1(plan(), p, p, p, 4, p, p, None, None, p, None))
    for kw, word in (({"a": None}, "point_sign_dev"), ({"b": None}, "dst_sign_dev"), ({"c": None}, "grad_loss_dev"), ({"d": None}, "grad_color_dev")):
        assert err(calls["shade_l1_backward"](plan(), **kw)).endswith(word + " is null"), kw

    def extract(fill, batch=1, V=3, T=1, H=8, W=8, rast=p, pos=p, prepared=p, tri=p, opp=p, out=p, n_blends=4):
        if fill:
            return lib.tsamd_shade_plan_fill(rast, pos, prepared, tri, opp, batch, V, T, H, W, out, n_blends, out, out, out, None)
        return lib.tsamd_shade_plan_count(rast, pos, prepared, tri, opp, batch, V, T, H, W, out, None)

    for fill in (False, True):
        for kw in ({"H": 8193}, {"W": 8193}, {"batch": -1}, {"H": -1}):
            assert "out of range (0 .. 8192 pixels per side)" in err(extract(fill, **kw)), (fill, kw)
        assert "below 2^30 pixels" in err(extract(fill, batch=1 << 20, H=64, W=64))
        for kw in ({"T": 1 << 24}, {"T": -1}, {"V": -1}):
            assert "2^24 - 1 triangles" in err(extract(fill, **kw)), (fill, kw)
        for name, word in (("rast", "rast_dev"), ("pos", "pos_clip_dev"), ("prepared", "prepared_dev"), ("tri", "tri_dev"), ("opp", "edge_partner_dev")):
            assert err(extract(fill, **{name: None})).endswith(word + " is null"), (fill, name)
    assert err(extract(False, out=None)).endswith("counts_out_dev is null")
    assert err(extract(True, out=None)).endswith("offsets_dev is null")
    assert "n_blends out of range" in err(extract(True, n_blends=-1))
    assert "n_blends out of range" in err(extract(True, n_blends=6 * 64 + 1))
    assert "at most 2^31 - 1" in err(extract(True, batch=1 << 14, H=200, W=200, n_blends=1 << 31))
    assert lib.tsamd_shade_l1_workspace_bytes(-1) == -1 and lib.tsamd_shade_l1_workspace_bytes(1 << 30) == -1
    sizes = [0, 1, 255, 256, 257, 4950, 1 << 20, 120 * 512 * 512, (1 << 30) - 1]
    got = [lib.tsamd_shade_l1_workspace_bytes(n) for n in sizes]
    assert all(b > 0 and b % 256 == 0 for b in got) and got == sorted(got) and got[-1] > got[0]


def test_shade_kernels_are_built_without_fp_contraction():
    """The image bound of tests/shade_oracle.py counts one rounding per difference, product and sum."""
    from tssplat_amd import _build
    assert "shade_kernels.hip" in _build.SOURCES and "shade_capi.cpp" in _build.SOURCES
    assert _build.SOURCE_FLAGS.get("shade_kernels.hip") == ["-ffp-contract=off"]


# ================================================================ GPU tier ================================================================

@functools.lru_cache(maxsize=None)
def _gpu_case(scene):
    """Everything the cases of one scene share, computed once and never modified: the GPU's own rast, its plan, the oracle's events,
    images and gradients on that rast, and one fused forward + backward."""
    import torch
    import tssplat_amd.dr as dr
    build, res = O.SCENES[scene]
    H, W = res
    pos_np, tri_np = build()
    pos, tri = torch.from_numpy(pos_np).cuda(), torch.from_numpy(tri_np).cuda()
    rast_d, _ = dr.rasterize(dr.RasterizeCudaContext(), pos, tri, resolution=[H, W], grad_db=False)
    rast = rast_d.cpu().numpy()
    events = R.antialias_events(rast, pos_np, tri_np)
    dst, src, wgt = O.records(events, H, W)
    _scene_condition(scene, rast, pos_np, tri_np, events, dst, src)
    plan = dr.plan_blends(rast_d, pos, tri)
    _, n_points = O.pix_point(rast)
    color_np, background_np, target_np = O.inputs(scene, n_points, rast.shape[:3])
    out64 = O.shade_csr(color_np, background_np, rast, dst, src, wgt)
    color = torch.from_numpy(color_np).cuda().requires_grad_(True)
    background, target = torch.from_numpy(background_np).cuda(), torch.from_numpy(target_np).cuda()
    upstream = torch.tensor(UPSTREAM, device="cuda")               # d objective / d loss lives on the device
    loss, image = dr.shade_l1(color, plan, background, target, return_image=True)
    (loss * upstream).backward()
    return dict(scene=scene, res=res, pos=pos, tri=tri, rast_d=rast_d, rast=rast, events=events, dst=dst, src=src, wgt=wgt, plan=plan, n_points=n_points,
                color_np=color_np, background_np=background_np, target_np=target_np, out64=out64, color=color, background=background, target=target,
                upstream=upstream, loss=loss.detach(), image=image, grad=color.grad.clone(), K=O.most_per_group(dst), Ks=O.most_per_group(src))


def _bits(t):
    import torch
    return t.detach().reshape(1).view(torch.int32).item()


def _rows(dst, src, wgt):
    rows = np.stack([np.asarray(dst, dtype=np.int64), np.asarray(src, dtype=np.int64), np.asarray(wgt, dtype=np.float32).view(np.int32).astype(np.int64)], axis=1)
    return rows[np.lexsort(rows.T[::-1])] if len(rows) else rows.reshape(0, 3)


def _assert_grouped_and_stable(perm, keys, group, ptr, slot_of_pixel):
    n = len(keys)
    assert np.array_equal(np.sort(perm), np.arange(n))
    k = keys[perm]
    assert np.all(np.diff(k) >= 0)
    assert np.all(np.diff(perm)[np.diff(k) == 0] > 0)             # stable: extraction order inside a group
    want_group, counts = np.unique(keys, return_counts=True)
    assert np.array_equal(group, want_group) and np.array_equal(ptr, np.concatenate([[0], np.cumsum(counts)]))
    if slot_of_pixel is not None:
        want_slot = np.full(len(slot_of_pixel), -1)
        want_slot[want_group] = np.arange(len(want_group))
        assert np.array_equal(slot_of_pixel, want_slot)


@pytest.mark.gpu
@pytest.mark.parametrize("scene", sorted(O.SCENES))
def test_plan_parity(scene):
    """pix_point is the prefix count of the GPU's own coverage; the records are the oracle's events on that rast as a multiset,
    weights equal as float32 bits; both CSR views are stable groupings of them; a second build gives the same bytes."""
    import torch
    import tssplat_amd.dr as dr
    c = _gpu_case(scene)
    plan = c["plan"]
    t = {k: v.cpu().numpy() for k, v in plan.tensors().items()}
    want_pp, n_points = O.pix_point(c["rast"])
    assert plan.n_points == n_points and plan.shape == c["rast"].shape[:3]
    assert np.array_equal(t["pix_point"], want_pp) and t["pix_point"].dtype == np.int32
    assert np.array_equal(t["point_pix"], np.nonzero(want_pp >= 0)[0])
    assert plan.n_blends == len(c["dst"]) and np.array_equal(_rows(t["rec_dst"], t["rec_src"], t["rec_weight"]), _rows(c["dst"], c["src"], c["wgt"]))
    # extraction order = pair slot order: destination / source pair (lower pixel, axis) never decreases
    lower = np.minimum(t["rec_dst"], t["rec_src"]).astype(np.int64)
    axis = (np.abs(t["rec_dst"].astype(np.int64) - t["rec_src"]) != 1).astype(np.int64)
    assert np.all(np.diff(2 * lower + axis) >= 0)
    n_pixels = len(want_pp)
    _assert_grouped_and_stable(t["dst_perm"], t["rec_dst"], t["dst_pix"], t["dst_ptr"], t["pix_dst"])
    _assert_grouped_and_stable(t["src_perm"], t["rec_src"], t["src_pix"], t["src_ptr"], None)
    assert np.array_equal(t["dst_src_pix"], t["rec_src"][t["dst_perm"]]) and np.array_equal(t["dst_weight"], t["rec_weight"][t["dst_perm"]])
    assert np.array_equal(t["dst_src_point"], want_pp[t["dst_src_pix"]])
    assert np.array_equal(t["src_dst_pix"], t["rec_dst"][t["src_perm"]]) and np.array_equal(t["src_weight"], t["rec_weight"][t["src_perm"]])
    assert np.array_equal(t["src_dst_slot"], t["pix_dst"][t["src_dst_pix"]])
    assert np.array_equal(t["point_dst"], t["pix_dst"][t["point_pix"]])
    src_slot = np.full(n_pixels, -1)
    src_slot[t["src_pix"]] = np.arange(len(t["src_pix"]))
    assert np.array_equal(t["point_src"], src_slot[t["point_pix"]])
    assert plan.nbytes == sum(v.nbytes for v in t.values()) and (plan.n_dst, plan.n_src) == (len(t["dst_pix"]), len(t["src_pix"]))
    again = dr.plan_blends(c["rast_d"], c["pos"], c["tri"])
    for name, a in plan.tensors().items():
        b = again.tensors()[name]
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), name


@pytest.mark.gpu
@pytest.mark.parametrize("scene", sorted(O.SCENES))
def test_image_and_loss(scene):
    """Per element |image - out64| <= image_bound(K), exactly equal where a pixel has no record; |loss - l1(out64)| <= loss_bound(K);
    dr.shade returns the same bits as shade_l1's image."""
    import torch
    import tssplat_amd.dr as dr
    c = _gpu_case(scene)
    image, out64, K = c["image"].cpu().numpy(), c["out64"], c["K"]
    assert image.shape == c["rast"].shape[:3] + (3,) and image.dtype == np.float32 and not c["image"].requires_grad
    err = np.abs(image - out64)
    want = O.l1(out64, c["target_np"])
    loss = float(c["loss"])
    print(f"shade {scene}: K = {K}, {len(c['dst'])} blends, image error {err.max():.3e} (bound {O.image_bound(K):.3e}), "
          f"loss {loss:.9g} against {want:.12g}: error {abs(loss - want):.3e} (bound {O.loss_bound(K):.3e})")
    assert np.all(err <= O.image_bound(K))
    untouched = np.ones(err.shape[:3], dtype=bool).reshape(-1)
    untouched[c["dst"]] = False
    assert np.array_equal(image.reshape(-1, 3)[untouched], out64.reshape(-1, 3)[untouched].astype(np.float32))
    assert c["loss"].dim() == 0 and c["loss"].dtype == torch.float32 and abs(loss - want) <= O.loss_bound(K)
    assert c["target_np"].shape[-1] == (4 if scene in O.FOUR_CHANNEL_TARGET else 3)
    with torch.no_grad():
        assert torch.equal(dr.shade(c["color"], c["plan"], c["background"]), c["image"])


@pytest.mark.gpu
@pytest.mark.parametrize("scene", sorted(O.SCENES))
def test_gradient(scene):
    """grad_color of shade_l1 with a device-side upstream gradient of 3 against the transposed form on the oracle's image, per entry
    within grad_bound(Kd, Ks, 3 / n); entries that read a sign the image bound cannot decide are left out, at most 0.1 % of them."""
    c = _gpu_case(scene)
    grad = c["grad"].cpu().numpy()
    assert grad.shape == (c["n_points"], 3)
    if c["n_points"] == 0:
        return
    g64 = O.l1_grad(c["out64"], c["target_np"], UPSTREAM)
    want = O.grad_color_csr(g64, c["rast"], c["dst"], c["src"], c["wgt"])
    excluded = _excluded_gradient_entries(_ambiguous(c["out64"], c["target_np"], c["K"]), c["rast"], c["dst"], c["src"])
    G = UPSTREAM / c["out64"].size
    # records on a point's own pixel as destination / as source
    bound = O.grad_bound(c["K"], c["Ks"], G)
    err = np.abs(grad - want)
    print(f"shade gradient {scene}: {excluded.sum()} of {excluded.size} entries excluded, |grad| max {np.abs(want).max():.3e}, "
          f"error / bound {err[~excluded].max() / bound:.3f}")
    assert excluded.mean() <= 1e-3 and np.abs(want).max() > 0
    assert np.all(err[~excluded] <= bound)


@pytest.mark.gpu
def test_sign_of_zero_is_zero():
    """Target = the composite itself: background pixels with target == background and foreground pixels with target == their colour
    have out - t == 0 exactly unless they are destinations; their loss terms and gradients are exactly zero (torch's sign(0) = 0),
    the rest matches the oracle."""
    import torch
    import tssplat_amd.dr as dr
    c = _gpu_case("checker_and_sheet")
    target_np = O.composite(c["color_np"], c["background_np"], c["rast"]).astype(np.float32)
    assert np.array_equal(target_np.astype(np.float64), O.composite(c["color_np"], c["background_np"], c["rast"]))
    color = torch.from_numpy(c["color_np"]).cuda().requires_grad_(True)
    loss = dr.shade_l1(color, c["plan"], c["background"], torch.from_numpy(target_np).cuda())
    (loss * c["upstream"]).backward()
    grad = color.grad.cpu().numpy()
    want_loss = O.l1(c["out64"], target_np)
    assert want_loss > 0 and abs(float(loss.detach()) - want_loss) <= O.loss_bound(c["K"])
    pp, _ = O.pix_point(c["rast"])
    is_dst = np.zeros(len(pp), dtype=bool)
    is_dst[c["dst"]] = True
    touched = is_dst.copy()
    touched[c["src"]] = True
    idle = ~touched[pp >= 0]
    assert idle.sum() > 1000 and (~idle).sum() > 100
    assert np.all(grad[idle] == 0.0)
    want = O.grad_color_csr(O.l1_grad(c["out64"], target_np, UPSTREAM), c["rast"], c["dst"], c["src"], c["wgt"])
    # (off the destinations out == target exactly in float32 and in float64: sign 0 on both sides, nothing to exclude; a destination
    # whose blend happens to cancel within the bound has a discrete sign like any other element)
    excluded = _excluded_gradient_entries(_ambiguous(c["out64"], target_np, c["K"]) & is_dst.reshape(c["out64"].shape[:3] + (1,)), c["rast"], c["dst"], c["src"])
    assert np.abs(want).max() > 0
    assert np.all(np.abs(grad - want)[~excluded] <= O.grad_bound(c["K"], c["Ks"], UPSTREAM / c["out64"].size))


@pytest.mark.gpu
@pytest.mark.parametrize("scene", sorted(O.SCENES))
def test_exact_invariants(scene):
    """A second call gives the same bits (loss, image, grad_color); the returned image as target gives loss 0.0 and a zero gradient
    exactly; dr.shade's backward fed with sign(out - t) s / n formed in torch from its own image equals shade_l1's grad_color."""
    import torch
    import tssplat_amd.dr as dr
    c = _gpu_case(scene)
    plan, background, target = c["plan"], c["background"], c["target"]
    color = c["color"].detach().clone().requires_grad_(True)
    loss, image = dr.shade_l1(color, plan, background, target, return_image=True)
    (loss * c["upstream"]).backward()
    assert _bits(loss) == _bits(c["loss"])
    assert torch.equal(image, c["image"]) and torch.equal(color.grad, c["grad"])
    with torch.no_grad():                                          # without a gradient: no sign arrays, same loss bits
        assert _bits(dr.shade_l1(color, plan, background, target)) == _bits(c["loss"])

    for tgt in (image, torch.cat([image, torch.rand_like(image[..., :1])], dim=-1)):
        color.grad = None
        zero = dr.shade_l1(color, plan, background, tgt.contiguous())
        (zero * c["upstream"]).backward()
        assert float(zero.detach()) == 0.0 and float(color.grad.abs().sum()) == 0.0

    color.grad = None
    own = dr.shade(color, plan, background)
    assert torch.equal(own.detach(), c["image"])
    n = torch.tensor(float(own.numel()), device="cuda")
    own.backward(torch.sign(own.detach() - target[..., :3]) * (c["upstream"] / n))
    assert torch.equal(color.grad, c["grad"])


def _renderer(**kw):
    import torch
    from tssplat_amd import geometry, materials, renderers
    m = np.load(os.path.join(ROOT, "tests", "golden", "mario_mesh.npz"))
    v, f = m["vertices"].astype(np.float32), m["faces"].astype(np.int32)
    geo = geometry.TetMeshGeometry(v, np.zeros((0, 4), np.int32), use_smooth_barrier=False, optimize_geo=False,
                                   surface_vid=np.arange(v.shape[0], dtype=np.int32), surface_fid=f)
    grid = dict(materials.ExplicitMaterial.Config(n_output_dims=3, material_activation="sigmoid").pos_encoding_config,
                n_levels=4, log2_hashmap_size=12)
    torch.manual_seed(0)
    mat = materials.ExplicitMaterial({"n_output_dims": 3, "material_activation": "sigmoid", "pos_encoding_config": grid})
    return renderers.MeshRasterizer(geo, mat, **kw)


@pytest.mark.gpu
def test_renderer_paths_agree_and_misuse_raises():
    """The frozen golden mesh with the real ExplicitMaterial, 3 views x 48^2, in the planned route: the operators path against
    MeshRasterizer(fused_shade=True) and against shade_loss.  ``shaded`` within twice the image bound, the loss within twice the
    loss bound (both paths are within one bound of the same float64 value), the loss falls over 30 steps in both fused modes.
    Misuse raises.

    The material's parameter gradients are held to 2e-5 of the tensor's largest entry.  That tolerance is this test's own: between
    its two grid routes tests/test_hashgrid_planned.py asks for equal bits, which cannot hold here -- the two image paths round
    grad_color differently (atomics in arbitrary order against a fixed order) -- and its 2e-5 is relative to the float64 oracle's sum
    of |terms| per entry, which this test has no oracle for.  2e-5 of the largest entry is the same factor on a scale that is no
    larger than that sum for the entry it is taken from; the target (half the rendered image) keeps every out - t far from 0, so
    no sign can differ between the paths."""
    import torch
    from tssplat_amd import dr, scenes
    from tssplat_amd.utils.optimizer import AdamUniform
    views, res = 3, 48
    mvp = torch.from_numpy(scenes.dataset_mvps(views).astype(np.float32)).cuda()
    bg = torch.rand(views, res, res, 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    loss_fn = torch.nn.L1Loss()
    rens = {"operators": _renderer(), "fused": _renderer(fused_shade=True), "fused-loss": _renderer()}
    assert rens["operators"].fused_shade is False and rens["fused"].fused_shade is True
    plans = {k: r.plan_views(mvp, res) for k, r in rens.items()}
    plan = plans["operators"]
    assert plan._blend_plan is None                                # lazy: nothing is built for a caller that does not ask
    bp = plans["fused"].blend_plan
    assert bp is plans["fused"].blend_plan and bp.n_points == plan.n_points > 500 and bp.n_blends >= 20 and bp.shape == (views, res, res)
    K = int(torch.diff(bp.dst_ptr).max())
    assert 1 <= K <= 4
    with torch.no_grad():
        plain = rens["operators"](mvp, only_alpha=False, iter_num=0, resolution=res, background=bg, view_plan=plan)["shaded"]
    target = torch.cat([(plain * 0.5), torch.ones_like(plain[..., :1])], dim=-1).contiguous()     # RGBA like the trainer's color_ref

    def run(mode, it=0):
        ren, vp = rens[mode], plans[mode]
        if mode == "fused-loss":
            out = ren.shade_loss(vp, bg, target, it)
            assert set(out) == {"img_loss", "geo_regularization", "shaded"} and not out["shaded"].requires_grad
            return out["img_loss"], out["shaded"]
        out = ren(mvp, only_alpha=False, iter_num=it, resolution=res, background=bg, view_plan=vp)
        return loss_fn(out["shaded"][..., :3], target[..., :3]), out["shaded"].detach()

    grads, shaded, losses = {}, {}, {}
    for mode, ren in rens.items():
        ren.zero_grad(set_to_none=True)
        loss, shaded[mode] = run(mode)
        (loss * 20).backward()
        losses[mode] = float(loss)
        grads[mode] = [p.grad.clone() for p in ren.materials.parameters()]
    for mode in ("fused", "fused-loss"):
        assert shaded[mode].shape == plain.shape
        d_img = float((shaded[mode] - shaded["operators"]).abs().max())
        d_loss = abs(losses[mode] - losses["operators"])
        worst = 0.0
        for a, b in zip(grads[mode], grads["operators"]):
            scale = float(b.abs().max())
            assert scale > 0
            worst = max(worst, float((a - b).abs().max()) / scale)
        print(f"renderer {mode}: shaded differs by {d_img:.3e} (bound {2 * O.image_bound(K):.3e}), loss by {d_loss:.3e} "
              f"(bound {2 * O.loss_bound(K):.3e}), parameter gradients by {worst:.3e} of the largest entry")
        assert d_img <= 2 * O.image_bound(K) and d_loss <= 2 * O.loss_bound(K) and worst <= 2e-5
    assert torch.equal(shaded["fused"], shaded["fused-loss"])
    for mode in ("fused", "fused-loss"):
        opt = AdamUniform(rens[mode].parameters(), lr=0.01)
        trace = []
        for it in range(30):
            loss, _ = run(mode, it)
            opt.zero_grad(set_to_none=True)
            (loss * 20).backward()
            opt.step()
            trace.append(loss.detach())
        trace = [float(l) for l in trace]
        assert trace[-1] < trace[0], (mode, trace)
    # fit_depth keeps working from the plan's rast
    campos = torch.tensor([[0.0, 1.0, 3.0]] * views, device="cuda")
    with torch.no_grad():
        a = rens["operators"](mvp, only_alpha=False, iter_num=0, resolution=res, background=bg, view_plan=plan, fit_depth=True, campos=campos)
        b = rens["fused"](mvp, only_alpha=False, iter_num=0, resolution=res, background=bg, view_plan=plans["fused"], fit_depth=True, campos=campos)
    assert torch.equal(a["d"], b["d"])

    fused, vp = rens["fused"], plans["fused"]
    with pytest.raises(RuntimeError, match="only_alpha"):
        fused(mvp, only_alpha=True, iter_num=0, resolution=res, background=bg, view_plan=vp)
    with pytest.raises(RuntimeError, match="permute_surface_scheduler"):
        fused(mvp, only_alpha=False, iter_num=0, resolution=res, background=bg, view_plan=vp, permute_surface_scheduler=lambda it: 0.01)
    with pytest.raises(RuntimeError, match="permute_surface_scheduler"):
        fused.shade_loss(vp, bg, target, 0, permute_surface_scheduler=lambda it: 0.01)
    with pytest.raises(RuntimeError, match="resolution"):
        fused(mvp, only_alpha=False, iter_num=0, resolution=64, background=bg, view_plan=vp)
    big = torch.ones(views, 64, 64, 3, device="cuda")
    with pytest.raises(RuntimeError, match="batch and resolution"):
        fused(mvp, only_alpha=False, iter_num=0, resolution=res, background=big, view_plan=vp)
    with pytest.raises(RuntimeError, match="batch and resolution"):
        fused.shade_loss(vp, big, target, 0)
    with pytest.raises(RuntimeError, match="batch and resolution"):
        fused.shade_loss(vp, bg, torch.ones(views, 64, 64, 4, device="cuda"), 0)
    color = torch.rand(bp.n_points + 1, 3, device="cuda")
    with pytest.raises(RuntimeError, match="n_points"):
        dr.shade(color, bp, bg)
    with pytest.raises(RuntimeError, match="n_points"):
        dr.shade_l1(color[:-2], bp, bg, target)
    with pytest.raises(RuntimeError, match="float32"):
        dr.shade(color[:-1].double(), bp, bg)
    with pytest.raises(RuntimeError, match="contiguous"):
        dr.shade_l1(color[:-1], bp, bg, target[..., :3])
    with pytest.raises(RuntimeError, match="BlendPlan"):
        dr.shade(color[:-1], vp, bg)
