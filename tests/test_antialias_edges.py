"""dr.antialias against the float64 oracle where tests/test_raster.py::test_antialias_forward_backward does not go: views that end
inside a 64-pixel chunk and inside a 256-pixel workgroup, images in which every pixel forms pairs, open and non-manifold meshes,
vertices that cannot be projected, ids that do not belong to the mesh, 2 and 4 channels, waves of the prepared form that own
more than one chunk, and the automatic choice between the two forms.

The CPU tests come first: the oracle's rule for foreign ids, and one test per scene builder (tests/aa_scenes.py) asserting --
with the oracle alone -- that the scene produces the case it exists for.  The GPU tests repeat the condition on the GPU's own
``rast`` before they look at a kernel.
"""
import numpy as np
import pytest

import aa_scenes as S
from oracle import raster_oracle as R

EPS = 2.0 ** -24     # unit round-off of float32


def masked_group(n_chunks):
    """Chunks per wave of the prepared kernels (``masked_launch`` in aa_kernels.hip, restated: a property of the launch, not of
    the result).  Group 64 needs 2^20 chunks -- 67 M pixels -- and stays uncovered by this file."""
    g = 1
    while g < 64 and n_chunks // (2 * g) >= 16384:
        g *= 2
    return g


def _blends_per_pixel(events):
    count = {}
    for ev in events:
        count[ev[0]] = count.get(ev[0], 0) + 1
    return count


def _events_by_edge_kind(events, tri, opp, ok):
    """(on boundary edges, on edges with three or more triangles, on edges one of whose partner vertices cannot be projected)"""
    slots = S.edge_slots(tri)
    boundary = fan = blind = 0
    for ev in events:
        s = slots[(min(ev[5]), max(ev[5]))]
        boundary += len(s) == 1
        fan += len(s) >= 3
        blind += any(0 <= opp[k] < len(ok) and not ok[opp[k]] for k in s)
    return boundary, fan, blind


def _skipped_for_a_vertex(rast_b, pos_b, tri):
    """Pairs of one view whose winning triangle has a vertex at w <= 0 / NaN: candidates that must blend nothing."""
    _, win = S.pair_winners(rast_b)
    win = win[(win >= 0) & (win < len(tri))]
    return int((~S.projectable(pos_b)[tri[win]]).any(axis=1).sum())


# ================================================================ CPU tier ================================================================

def test_oracle_antialias_skips_foreign_ids():
    """A rast image whose ids do not belong to the triangle list, a triangle with a vertex index outside the position array and a
    partner entry outside it: the pair is skipped / the edge has no partner, and nothing is indexed with such a value (numpy
    would raise on ``tri[t]`` and wrap a negative index silently)."""
    H, W = 6, 8
    pos, tri = S.checker(H, W, 1, 1, 3, 4, seed=1)                            # 12 quads, 24 triangles, quad q owns vertices 4 q .. 4 q + 3
    rast = R.rasterize(pos, tri, (H, W))
    full = R.antialias_events(rast, pos, tri)[0]
    col = np.random.default_rng(0).random((1, H, W, 3)).astype(np.float32)
    # (a) the triangle list truncated to the first six quads: pairs won by a later quad's triangle are foreign
    T, kept = 12, set(range(24))
    _, win = S.pair_winners(rast[0])
    assert (win >= T).sum() >= 5 and ((win >= 0) & (win < T)).sum() >= 5
    cut = R.antialias_events(rast, pos, tri[:T])[0]
    assert 3 <= len(cut) < len(full)
    assert all(set(ev[5]) <= kept for ev in cut)                              # every blend on an edge of a kept quad
    assert [ev for ev in full if set(ev[5]) <= kept] == cut                   # and exactly those the full list gives there
    # (b) a vertex index beyond the position array (and a negative one): that triangle's pairs are skipped, the rest stands
    for bad in (pos.shape[1], 10 ** 6, -1, -3):
        edited = tri.copy()
        t_bad = next(t for t in win.tolist() if 0 <= t < T and any(set(ev[5]) <= set(tri[t].tolist()) for ev in full))
        edited[t_bad, 1] = bad
        ev = R.antialias_events(rast, pos, edited)[0]
        assert len(ev) < len(full)
        ref = R.antialias(col, rast, pos, edited)
        gc, gp = R.antialias_backward(col, rast, pos, edited, np.ones_like(col))
        assert np.isfinite(ref).all() and np.isfinite(gc).all() and np.isfinite(gp).all()
    # (c) a partner entry outside [0, V) is "no partner": the same events as with -1 there
    opp = R.edge_partners(tri)
    shared = np.nonzero(opp >= 0)[0]
    assert len(shared) == 24                                                  # the twelve diagonals, seen from both sides
    for bad in (pos.shape[1], 2 ** 31 - 1, -7):
        o_bad, o_none = opp.copy(), opp.copy()
        o_bad[shared], o_none[shared] = bad, -1
        assert R.antialias_events(rast, pos, tri, o_bad) == R.antialias_events(rast, pos, tri, o_none)
        assert len(R.antialias_events(rast, pos, tri, o_none)[0]) > len(full)     # (the diagonals blend once they have no partner)
    # the image and the gradients follow the events: nothing blended, nothing scattered for the skipped pairs
    ref = R.antialias(col, rast, pos, tri[:T])
    touched = {ev[0] for ev in cut}
    for j in range(H):
        for i in range(W):
            assert ((j, i) in touched) == bool(np.any(ref[0, j, i] != col[0, j, i].astype(np.float64)))
    _, gp = R.antialias_backward(col, rast, pos, tri[:T], np.ones_like(col))
    assert np.all(gp[0, 24:] == 0.0) and np.any(gp[0, :24] != 0.0)


def test_scene_checker_fills_chunks_and_pixels():
    """``checker`` exists for pair density: chunks with all 128 mask bits set, a pair list of more than 256 items in a
    256-pixel workgroup (a second round of its analysis loop; 140 of 160 columns give at most 473 of the 512 a list can
    hold), pixels that receive two blends, boundary edges only."""
    H, W = 24, 160
    pos, tri = S.checker(H, W, 9, 10, 6, 140, views=2)
    rast = R.rasterize(pos, tri, (H, W))
    assert len(np.unique(rast[0, ..., 3])) == 6 * 140 + 1                     # one triangle of every quad, and the background
    per_chunk = S.pairs_per_chunk(rast)
    assert (per_chunk == 128).sum() >= 8 and (per_chunk >= 100).sum() >= 20
    per_workgroup = per_chunk[:len(per_chunk) // 4 * 4].reshape(-1, 4).sum(axis=1)
    assert per_workgroup.max() >= 400
    opp = R.edge_partners(tri)
    assert (opp >= 0).sum() == 2 * 6 * 140                                    # the diagonals; every outer edge is a boundary
    for b, events in enumerate(R.antialias_events(rast, pos, tri, opp)):
        assert len(events) > 800
        assert max(_blends_per_pixel(events).values()) == 2
        boundary, _, _ = _events_by_edge_kind(events, tri, opp, S.projectable(pos[b]))
        assert boundary == len(events)


def _comb_scene(H, W, views):
    return S.merge(S.comb(H, W, 1, 4, 150, 10, axis=1, views=views, seed=1), S.comb(H, W, 12, 4, 11, 150, axis=0, views=views, seed=2))


def test_scene_comb_piles_events_on_few_vertices():
    """``comb`` exists for the atomics on ``grad_pos``: a long strip's vertices take one contribution per pixel of its length,
    on both axes."""
    H, W = 24, 160
    pos, tri = _comb_scene(H, W, 2)
    rast = R.rasterize(pos, tri, (H, W))
    for events in R.antialias_events(rast, pos, tri):
        per_vertex = np.zeros((2, pos.shape[1]), dtype=np.int64)
        for ev in events:
            per_vertex[ev[4], list(ev[5])] += 1
        assert per_vertex[1].max() >= 100                                     # horizontal strips, 150 pixels long: vertical pairs
        assert per_vertex[0].max() >= 8                                       # vertical strips, 11 pixels long: horizontal pairs
        assert (per_vertex[0] > 0).sum() >= 200


def test_scene_open_sheet_has_boundary_and_fold_silhouettes():
    """``open_sheet`` exists for ``opp = -1`` and for silhouette edges that DO have a partner (the folds)."""
    H, W = 48, 64
    pos, tri = S.open_sheet(H, W, views=2)
    opp = R.edge_partners(tri)
    assert (opp < 0).sum() == 2 * (12 - 1) + 2 * (10 - 1)
    rast = R.rasterize(pos, tri, (H, W))
    for b, events in enumerate(R.antialias_events(rast, pos, tri, opp)):
        boundary, fan, _ = _events_by_edge_kind(events, tri, opp, S.projectable(pos[b]))
        assert boundary >= 100 and len(events) - boundary >= 30 and fan == 0


def test_scene_soup_has_every_irregular_case():
    """``soup`` exists for what a clean mesh never shows: events on boundary edges and on an edge with three triangles, pairs
    skipped because their triangle has a vertex at w <= 0 / NaN, and an edge that blends although it has a partner, because
    the partner's far vertex cannot be projected."""
    H, W = 48, 64
    pos, tri = S.soup(H, W)
    assert np.array_equal(pos[1], pos[0][::-1], equal_nan=True)
    slots = S.edge_slots(tri)
    assert len(slots[S.SOUP_FAN]) >= 3
    assert any(len(set(r)) < 3 for r in tri.tolist())                         # a degenerate triangle
    assert len({tuple(r) for r in tri.tolist()}) <= len(tri) - 10             # duplicates
    ok0 = S.projectable(pos[0])
    assert not ok0[list(S.SOUP_BEHIND)].any() and not ok0[S.SOUP_NAN] and ok0[S.SOUP_FAR]
    assert abs(pos[0, S.SOUP_FAR, 0] / pos[0, S.SOUP_FAR, 3] * 0.5 + 0.5) * W > 16384        # beyond the guard band
    rast = R.rasterize(pos, tri, (H, W))
    opp = R.edge_partners(tri)
    events = R.antialias_events(rast, pos, tri, opp)
    kinds = np.array([_events_by_edge_kind(events[b], tri, opp, S.projectable(pos[b])) for b in range(2)])
    assert kinds[:, 0].min() >= 50 and kinds[:, 1].sum() >= 3 and kinds[:, 2].sum() >= 1
    assert min(_skipped_for_a_vertex(rast[b], pos[b], tri) for b in range(2)) >= 100


# ================================================================ GPU tier ================================================================

class _Spy:
    """The loaded library with the antialias entry points recorded: which form a call of ``dr.antialias`` took."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in ("tsamd_antialias_prepare", "tsamd_antialias", "tsamd_antialias_backward"):
            return fn

        def recorded(*args):
            self.calls.append((name, args))
            return fn(*args)
        return recorded

    def took(self):
        """("resolve-masks" | "scan-masks" | "per-pair") of the calls recorded so far; asserts they are consistent."""
        prep = [a for n, a in self.calls if n == "tsamd_antialias_prepare"]
        fwd = [a for n, a in self.calls if n == "tsamd_antialias"]
        assert len(fwd) == 1 and len(prep) <= 1
        assert (fwd[0][3] is not None) == (len(prep) == 1)
        if not prep:
            return "per-pair"
        return "scan-masks" if prep[0][4] is None else "resolve-masks"


ROUTES = ("resolve-masks", "scan-masks", "per-pair", "c-abi")


def _run_route(route, monkeypatch, pos_np, tri_np, res, col_np, g_np, boost, aa_tri_np, first_rast):
    """One forward + backward through ``route``; returns (rast as a tensor, out, grad_color, grad_pos as numpy, the form the call took)."""
    import torch
    import tssplat_amd.dr as dr
    from tssplat_amd import _capi
    tri_d = torch.from_numpy(tri_np).cuda()
    aa_tri_d = tri_d if aa_tri_np is tri_np else torch.from_numpy(aa_tri_np).cuda()
    with monkeypatch.context() as mp:
        mp.setattr(dr, "PAIR_MASKS_FROM_RASTERIZE", route != "scan-masks")
        if not route.startswith("default:"):                 # ("default:<the form expected>": the rule of _AntialiasFunc.forward decides)
            mp.setattr(dr, "PREPARE_ANTIALIAS", route in ("resolve-masks", "scan-masks"))
        dr._last_pair_masks.clear()
        dr._pair_masks_wanted.clear()                # (absent: the next rasterize call makes the masks if it may)
        spy = _Spy(dr._lib)
        mp.setattr(dr, "_lib", spy)
        pos = torch.from_numpy(pos_np).cuda().requires_grad_(True)
        rast, _ = dr.rasterize(dr.RasterizeCudaContext(), pos, tri_d, resolution=list(res), grad_db=False)
        if first_rast is not None:
            assert torch.equal(rast.detach(), first_rast)
        g = torch.from_numpy(g_np).cuda()
        if route == "c-abi":
            lib = _capi.load()
            topo = dr.antialias_construct_topology_hash(aa_tri_d)
            B, H, W, Cn = col_np.shape
            cd, pd, rd = torch.from_numpy(col_np).cuda(), pos.detach().contiguous(), rast.detach().contiguous()
            out, gc, gp = torch.empty_like(cd), torch.empty_like(cd), torch.empty_like(pd)
            _capi.check(lib.tsamd_antialias(cd.data_ptr(), rd.data_ptr(), pd.data_ptr(), None, aa_tri_d.data_ptr(), topo.opp.data_ptr(), B, pd.shape[1],
                                            aa_tri_d.shape[0], H, W, Cn, out.data_ptr(), None))
            _capi.check(lib.tsamd_antialias_backward(cd.data_ptr(), rd.data_ptr(), pd.data_ptr(), None, aa_tri_d.data_ptr(), topo.opp.data_ptr(), B,
                                                     pd.shape[1], aa_tri_d.shape[0], H, W, Cn, g.data_ptr(), boost, gc.data_ptr(), gp.data_ptr(), None))
            torch.cuda.synchronize()
            return rast.detach(), out.cpu().numpy(), gc.cpu().numpy(), gp.cpu().numpy(), "c-abi"
        col = torch.from_numpy(col_np).cuda().requires_grad_(True)
        out = dr.antialias(col, rast, pos, aa_tri_d, topology_hash=None, pos_gradient_boost=boost)
        out.backward(g)
        # rast's (u, v) carry no gradient here (out does not depend on them), so pos.grad is the antialias term alone
        return rast.detach(), out.detach().cpu().numpy(), col.grad.cpu().numpy(), pos.grad.cpu().numpy(), spy.took()


def check_antialias(monkeypatch, pos_np, tri_np, res, channels, condition, min_changed, *, dense, routes=ROUTES, aa_tri_np=None, seed=7, boost=2.0):
    """The one comparison every case goes through.

    ``rast`` comes from dr.rasterize on the GPU (with ``tri_np``) and is handed to the oracle; ``condition(rast, events, opp)``
    asserts on it what the scene is there for, before any kernel output is looked at.  Then, per route: the image within 2e-6
    absolute of R.antialias (colours in [0, 1]; a blend costs three roundings of values <= 1 and a pixel receives at most four,
    asserted, so 4 * 3 * 2^-24 = 7e-7 is the worst rounding and a different decision shows as ~0.1) and bit-equal to the colour
    where the oracle blends nothing; grad_color within 1e-5 max(1, |gc|max); grad_pos within 2e-5 |gp|max for sparse scenes and,
    for ``dense`` ones, per entry within ``2^-24 (n + C + 2) M + 1e-30`` -- M the sum of the absolute values of the terms the
    entry is made of, n their number: n fp32 atomic additions, one rounding of every term, a C-term fp32 dot product -- and
    exactly zero on vertices no event touches.  Routes are held to the same bounds against each other."""
    aa_tri_np = tri_np if aa_tri_np is None else aa_tri_np
    B, V = pos_np.shape[:2]
    H, W = res
    rng = np.random.default_rng(seed)
    col_np = rng.random((B, H, W, channels), dtype=np.float32)
    g_np = rng.standard_normal((B, H, W, channels), dtype=np.float32)
    results, rast_d = {}, None
    for route in routes:
        r = _run_route(route, monkeypatch, pos_np, tri_np, res, col_np, g_np, boost, aa_tri_np, rast_d)
        rast_d = r[0]
        assert r[4] == route.split(":")[-1], (r[4], route)
        results[route] = r[1:4]
    rast_np = rast_d.cpu().numpy()
    del rast_d

    # ---- the oracle, one view at a time (the large cases stay flat in host memory) ----
    opp = R.edge_partners(aa_tri_np)
    ref = np.empty((B, H, W, channels))
    gc = np.empty((B, H, W, channels))
    gp = np.empty((B, V, 4))
    mass = np.zeros((B, V, 4))
    count = np.zeros((B, V))
    untouched = np.ones((B, H, W), dtype=bool)
    events = []
    for b in range(B):
        sl = slice(b, b + 1)
        ev = R.antialias_events(rast_np[sl], pos_np[sl], aa_tri_np, opp)
        events.append(ev[0])
        ref[sl] = R.antialias(col_np[sl], rast_np[sl], pos_np[sl], aa_tri_np, opp, events=ev)
        gc[sl], gp[sl] = R.antialias_backward(col_np[sl], rast_np[sl], pos_np[sl], aa_tri_np, g_np[sl], opp, pos_gradient_boost=boost, events=ev)
        p64, c64, g64 = pos_np[b].astype(np.float64), col_np[b].astype(np.float64), g_np[b].astype(np.float64)
        for dst, src, _, _, _, (va, vb), (dA, dB) in ev[0]:
            untouched[b][dst] = False
            a = abs(boost) * float(np.sum(np.abs(g64[dst]) * np.abs(c64[src] - c64[dst])))
            for vtx, (ddx, ddy) in ((va, dA), (vb, dB)):
                x, y, _, w = p64[vtx]
                gx, gy = a * abs(ddx) * (0.5 * W / w), a * abs(ddy) * (0.5 * H / w)
                mass[b, vtx, 0] += gx
                mass[b, vtx, 1] += gy
                mass[b, vtx, 3] += (gx * abs(x) + gy * abs(y)) / w
                count[b, vtx] += 1

    condition(rast_np, events, opp)
    assert max(max(_blends_per_pixel(ev).values(), default=0) for ev in events) <= 4
    n_changed = int((np.abs(ref - col_np).sum(-1) > 0).sum())
    print(f"antialias case {B}x{H}x{W}x{channels}: {sum(len(e) for e in events)} blends on {n_changed} pixels, "
          f"{int(S.differing_pairs(rast_np).sum())} pairs, at most {int(count.max())} events on a vertex")
    assert n_changed >= min_changed
    assert np.abs(gp).max() > 0

    tol_out = 2e-6
    tol_gc = 1e-5 * max(1.0, np.abs(gc).max())
    tol_gp = EPS * (count[..., None] + channels + 2) * mass + 1e-30 if dense else np.full(gp.shape, 2e-5 * np.abs(gp).max())
    tol_gp = np.where(count[..., None] > 0, tol_gp, 0.0)
    first = None
    for route, (out, gcol, gpos) in results.items():
        for name, got, want, tol in (("out", out, ref, tol_out), ("grad_color", gcol, gc, tol_gc), ("grad_pos", gpos, gp, tol_gp)):
            err = np.abs(got - want)
            print(f"  {route:14s} {name:10s} max error {err.max():.3e}, largest error / bound {np.max(err / np.maximum(tol, 1e-300)):.3f}")
            assert np.all(err <= tol), (route, name)
        assert np.array_equal(out[untouched], col_np[untouched]), route
        if first is None:
            first = (out, gcol, gpos)
        else:
            assert np.all(np.abs(out - first[0]) <= tol_out) and np.all(np.abs(gcol - first[1]) <= tol_gc) and np.all(np.abs(gpos - first[2]) <= tol_gp), route


def _ragged(res, views=None):
    H, W = res
    if (H, W) == (33, 50):
        return S.merge(S.checker(H, W, 27, 3, 6, 47, views=views or 3), S.open_sheet(H, W, views=views or 3, box=(2, -1, 48, 25)))
    return S.merge(S.checker(H, W, 0, 0, 3, 191, views=views or 2), S.open_sheet(H, W, nu=30, nv=5, views=views or 2, box=(1, 3.5, 191, 7.5)))


@pytest.mark.gpu
@pytest.mark.parametrize("views,res", [(3, (33, 50)), (2, (7, 192))])
def test_antialias_on_views_that_end_inside_a_chunk(views, res, monkeypatch):
    """Views that end inside a 64-pixel chunk (33 x 50) or inside a 256-pixel workgroup of the per-pair form (both sizes): the
    chunk / workgroup holds the end of one view and the start of the next, the batch ends in a partial chunk (3 x 33 x 50), pairs
    lie in the last row and the last column of a view (the ``i + 1 < width`` / ``j + 1 < height`` guards), and the views
    differ, so that a per-view base (rast, pos, windows, flags) taken from the wrong side of a straddling chunk shows."""
    H, W = res
    pos, tri = _ragged(res)
    units = [u for u in (64, 256) if (H * W) % u != 0]
    assert units == ([64, 256] if res == (33, 50) else [256])
    assert ((views * H * W) % 64 != 0) == (res == (33, 50))

    def condition(rast, events, opp):
        flat = S.differing_pairs(rast).reshape(-1, 2).any(axis=1)
        for unit in units:
            for b in range(1, views):                                         # the chunk / workgroup that straddles views b - 1 | b: pairs on both sides
                k = b * H * W // unit
                assert flat[unit * k:b * H * W].any() and flat[b * H * W:unit * (k + 1)].any()
        if (views * H * W) % 64 != 0:
            assert S.pairs_per_chunk(rast)[-1] > 0                            # the partial chunk at the end
        ids = rast[..., 3]
        # without the guards the last column would pair with the next row's first pixel, the last row with the next view's first
        assert (ids[:, :-1, -1] != ids[:, 1:, 0]).any() and (ids[:-1, -1, :] != ids[1:, 0, :]).any()
        assert all(len(ev) > 200 for ev in events)

    check_antialias(monkeypatch, pos, tri, res, 3, condition, 400, dense=False)


@pytest.mark.gpu
@pytest.mark.parametrize("channels", [1, 4])
@pytest.mark.parametrize("scene", ["checker", "comb"])
def test_antialias_on_dense_pair_images(scene, channels, monkeypatch):
    """One chunk per wave, but full: 128-bit mask chunks and pair lists beyond 256 items (checker), two blends per pixel, and vertices
    that take more than a hundred atomic contributions (comb) -- with grad_pos held to its rounding-error bound per entry."""
    H, W = 24, 160
    pos, tri = S.checker(H, W, 9, 10, 6, 140, views=2) if scene == "checker" else _comb_scene(H, W, 2)

    def condition(rast, events, opp):
        per_chunk = S.pairs_per_chunk(rast)
        assert max(max(_blends_per_pixel(ev).values()) for ev in events) == 2
        if scene == "checker":
            assert (per_chunk == 128).sum() >= 8
            assert per_chunk[:len(per_chunk) // 4 * 4].reshape(-1, 4).sum(axis=1).max() >= 400
        else:
            n = np.zeros(pos.shape[:2])
            for b, ev in enumerate(events):
                for e in ev:
                    n[b, list(e[5])] += 1
            assert n.max() >= 100

    check_antialias(monkeypatch, pos, tri, (H, W), channels, condition, 1000, dense=True)


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["open_sheet", "soup"])
def test_antialias_on_open_and_non_manifold_meshes(scene, monkeypatch):
    """Boundary edges (``opp = -1``: always a silhouette), edges with three triangles (partner = lowest other id), triangles
    with a vertex at w <= 0 / NaN (the pair is skipped, edge flags 0: the silhouette of a clipped triangle is not antialiased)
    and partners whose far vertex cannot be projected (no partner); 2 channels."""
    H, W = 48, 64
    pos, tri = S.open_sheet(H, W, views=2) if scene == "open_sheet" else S.soup(H, W)

    def condition(rast, events, opp):
        kinds = np.array([_events_by_edge_kind(events[b], tri, opp, S.projectable(pos[b])) for b in range(2)])
        assert kinds[:, 0].min() >= 50                                        # events on boundary edges, in every view
        if scene == "open_sheet":
            assert (np.array([len(ev) for ev in events]) - kinds[:, 0]).min() >= 30      # and on folds, which have a partner
        else:
            assert kinds[:, 1].sum() >= 3 and kinds[:, 2].sum() >= 1
            assert min(_skipped_for_a_vertex(rast[b], pos[b], tri) for b in range(2)) >= 100

    check_antialias(monkeypatch, pos, tri, (H, W), 2, condition, 200 if scene == "soup" else 300, dense=False)


@pytest.mark.gpu
def test_antialias_skips_foreign_ids_on_gpu(monkeypatch):
    """``rast`` made with a longer triangle list than antialias is given, and one remaining triangle edited to a vertex index
    >= V: pairs won by such triangles blend nothing, a partner entry >= V counts as no partner -- the oracle's rule
    (test_oracle_antialias_skips_foreign_ids), on all four routes.  (A read through one of those indices would land far outside
    the buffers: the edited index is 2^30.)"""
    H, W = 32, 32
    pos, tri = S.merge(S.open_sheet(H, W, nu=9, nv=8, views=1), S.checker(H, W, 12, 4, 8, 24, views=1))
    T = len(tri) - 2 * 8 * 24 + 2 * 8 * 12                                    # the sheet and half of the quads stay
    aa_tri = tri[:T].copy()
    edited = 2 * 4 * 8 + 1                                                    # a triangle in the middle of the sheet that wins pairs
    aa_tri[edited, 2] = 2 ** 30

    def condition(rast, events, opp):
        _, win = S.pair_winners(rast[0])
        assert (win >= T).sum() >= 100 and (win == edited).sum() >= 1 and ((win >= 0) & (win < T)).sum() >= 100
        assert (opp == 2 ** 30).sum() >= 1                                    # the edited vertex is somebody's partner
        assert len(events[0]) >= 100

    check_antialias(monkeypatch, pos, tri, (H, W), 3, condition, 100, dense=False, aa_tri_np=aa_tri)


@pytest.mark.gpu
@pytest.mark.parametrize("views,side,band,group,routes", [(2, 1025, (5, 330), 2, ROUTES), (1, 2049, (5, 600), 4, ("scan-masks",)),
                                                          (4, 2049, (2, 1300), 16, ("resolve-masks",))])
def test_antialias_with_waves_that_own_several_chunks(views, side, band, group, routes, monkeypatch):
    """Images large enough for ``masked_group`` > 1 -- 16 is what 120 views x 512^2 run with -- and a band of unit quads whose
    chunks are full: a wave pushes chunk after chunk on its 192-entry stack, pops the top 64, unpacks ``(c << 7) | (lane << 1) |
    axis`` with c > 0, and the last wave's chunks end before its group does.  The band starts at pixel (500, 300) in every view;
    it is 5 x 330 for group 2 and wider (5 x 600, 2 x 1300) for groups 4 and 16, because a wave's 4 / 16 chunks are 256 / 1024
    consecutive pixels of a row and a dense group-aligned run must fit in the band (two rows keep the oracle's time down).  Groups 4 and 16 take the prepared route only
    (the one a small mesh in a large image takes); the group-2 image also goes through the per-pair kernels.  Group 64 needs
    67 M pixels and stays uncovered."""
    H = W = side
    pos, tri = S.checker(H, W, 500, 300, band[0], band[1], views=views)
    n_chunks = (views * H * W + 63) // 64
    assert masked_group(n_chunks) == group
    assert n_chunks % group != 0 and (views * H * W) % 64 != 0               # the last wave is short of chunks, the last chunk of pixels
    assert 4 * (pos.shape[1] + len(tri)) <= H * W                             # and the automatic choice is the prepared form too

    def condition(rast, events, opp):
        per_chunk = S.pairs_per_chunk(rast)
        assert len(per_chunk) == n_chunks
        runs, deepest = S.dense_aligned_runs(per_chunk, group, at_least=100)
        print(f"group {group}: {n_chunks} chunks, {runs} waves with >= 100 pairs in every chunk, deepest {deepest} pairs")
        assert runs >= 1 and deepest >= 100 * group
        if "per-pair" in routes:
            assert per_chunk[:n_chunks // 4 * 4].reshape(-1, 4).sum(axis=1).max() >= 400      # a PairList filled well past one round

    check_antialias(monkeypatch, pos, tri, (H, W), 1, condition, 150 * band[0] * views, dense=True, routes=routes)


@pytest.mark.gpu
@pytest.mark.parametrize("prepared", [True, False])
def test_antialias_default_choice_of_form(prepared, monkeypatch):
    """``PREPARE_ANTIALIAS = None``: the prepared form exactly up to 4 (V + T) == H W, the per-pair form from one vertex more;
    the oracle's image either way."""
    H, W = 64, 64
    pos, tri = S.open_sheet(H, W, nu=14, nv=12, views=1)
    pad = H * W // 4 - (pos.shape[1] + len(tri)) + (0 if prepared else 1)
    assert pad > 0
    filler = np.tile(np.array([0.0, 0.0, 0.0, 1.0], dtype=np.float32), (1, pad, 1))
    pos = np.concatenate([pos, filler], axis=1)
    assert (4 * (pos.shape[1] + len(tri)) <= H * W) == prepared
    import tssplat_amd.dr as dr
    assert dr.PREPARE_ANTIALIAS is None
    check_antialias(monkeypatch, pos, tri, (H, W), 3, lambda rast, events, opp: None, 200, dense=False,
                    routes=("default:resolve-masks" if prepared else "default:per-pair",))


@pytest.mark.gpu
@pytest.mark.parametrize("res", [(7, 192), (33, 50)])
def test_antialias_skips_mask_bits_outside_the_image(res):
    """``pair_masks_dev`` is the caller's memory: through tsamd_antialias_prepare -> tsamd_antialias -> tsamd_antialias_backward, a
    bit for a pair that does not exist -- axis 0 in the last column, axis 1 in the last row (its second pixel lies past the end of
    the one view), any bit of a pixel past the end of the image -- is skipped by the pair driver, so the results are those of the
    rasteriser's own masks within the route-to-route tolerances of tests/test_raster.py::test_antialias_forward_backward.
    One view of 7 x 192 is 21 full chunks: its masks hold no pixel past the end, the last row's pairs are the ones that reach
    there.  One view of 33 x 50 ends inside a chunk, whose bits 50 .. 63 are set too."""
    import torch
    import tssplat_amd.dr as dr
    from tssplat_amd import _capi
    lib = _capi.load()
    H, W = res
    pos_np, tri_np = _ragged(res, views=1)
    pos, tri = torch.from_numpy(pos_np).cuda(), torch.from_numpy(tri_np).cuda()
    V, T, Cn = int(pos.shape[1]), int(tri.shape[0]), 3
    opp = dr.antialias_construct_topology_hash(tri).opp
    ws = torch.empty(int(lib.tsamd_rasterize_workspace_bytes(1, V, H, W)), dtype=torch.uint8, device="cuda")
    rast = torch.empty((1, H, W, 4), dtype=torch.float32, device="cuda")
    masks = torch.zeros(int(lib.tsamd_pair_masks_bytes(1, H, W)), dtype=torch.uint8, device="cuda")
    _capi.check(lib.tsamd_rasterize(pos.data_ptr(), 1, V, tri.data_ptr(), T, H, W, ws.data_ptr(), rast.data_ptr(), masks.data_ptr(), None))
    clean = masks.cpu().numpy().view(np.uint64).reshape(-1, 2).copy()
    assert len(clean) == (H * W + 63) // 64 and ((H * W) % 64 == 0) == (res == (7, 192))

    pix = np.arange(H * W)
    past = np.arange(H * W, 64 * len(clean))
    outside = (np.concatenate([pix[pix % W == W - 1], past]), np.concatenate([pix[pix // W == H - 1], past]))
    bad = clean.copy()
    for axis, idx in enumerate(outside):
        bit = np.uint64(1) << (idx & 63).astype(np.uint64)
        assert not (clean[idx >> 6, axis] & bit).any()                        # the rasteriser never names such a pair
        np.bitwise_or.at(bad[:, axis], idx >> 6, bit)
    assert len(outside[0]) >= H and len(outside[1]) >= W and (len(past) > 0) == (res == (33, 50))
    assert int(np.sum(clean != 0)) > 10                                       # and the image has pairs of its own

    rng = np.random.default_rng(7)
    col = torch.from_numpy(rng.random((1, H, W, Cn), dtype=np.float32)).cuda()
    g = torch.from_numpy(rng.standard_normal((1, H, W, Cn), dtype=np.float32)).cuda()
    prepared = torch.empty(int(lib.tsamd_antialias_prepared_bytes(1, V, T, H, W)), dtype=torch.uint8, device="cuda")

    def run(mask_words):
        m = torch.from_numpy(mask_words.view(np.uint8).reshape(-1).copy()).cuda()
        out, gc, gp = torch.empty_like(col), torch.empty_like(col), torch.empty_like(pos)
        _capi.check(lib.tsamd_antialias_prepare(None, pos.data_ptr(), tri.data_ptr(), opp.data_ptr(), m.data_ptr(), 1, V, T, H, W, prepared.data_ptr(), None))
        _capi.check(lib.tsamd_antialias(col.data_ptr(), rast.data_ptr(), pos.data_ptr(), prepared.data_ptr(), tri.data_ptr(), opp.data_ptr(), 1, V, T, H, W, Cn,
                                        out.data_ptr(), None))
        _capi.check(lib.tsamd_antialias_backward(col.data_ptr(), rast.data_ptr(), pos.data_ptr(), prepared.data_ptr(), tri.data_ptr(), opp.data_ptr(), 1, V, T, H, W,
                                                 Cn, g.data_ptr(), 2.0, gc.data_ptr(), gp.data_ptr(), None))
        torch.cuda.synchronize()
        return out.cpu().numpy(), gc.cpu().numpy(), gp.cpu().numpy()

    out0, gc0, gp0 = run(clean)
    out1, gc1, gp1 = run(bad)
    assert int((out0 != col.cpu().numpy()).any(axis=-1).sum()) > 100 and np.abs(gp0).max() > 0      # the clean run blends
    assert np.abs(out1 - out0).max() <= 1e-6
    assert np.abs(gc1 - gc0).max() <= 1e-5 * max(1.0, np.abs(gc0).max())
    assert np.abs(gp1 - gp0).max() <= 2e-5 * np.abs(gp0).max()
