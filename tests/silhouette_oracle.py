"""Oracle of the alpha stage (dr.silhouette, dr.silhouette_mse): numpy only, composed of oracle/raster_oracle.py.

The specification is the operators path of MeshRasterizer.forward(only_alpha=True) -- ``rasterize``, the id channel clipped to
[0, 1], ``antialias`` of that one-channel image and its backward -- plus a float64 mean squared error.  What the fused kernels rely
on is stated here as a filter: with colours in {0, 1} only the events of pairs with exactly one background pixel ("coverage
events") change anything; tests/test_silhouette.py asserts that on the CPU before any kernel is looked at.

``sparse_checker`` joins the scene builders of tests/aa_scenes.py: the plain ``checker`` is solid, so its coverage pairs lie on
its perimeter only.
"""
from __future__ import annotations

import numpy as np

import aa_scenes as S
from oracle import raster_oracle as R


def sparse_checker(H, W, j0, i0, nj, ni, off=(0.3, 0.3), views=1, seed=0):
    """Separate unit-pixel quads on every second pixel of the ``nj x ni`` band from pixel ``(j0, i0)`` on, in both directions (the
    black fields of a chessboard), shifted by ``off`` pixels, a random depth per quad and view; view ``b`` is shifted by a
    further ``0.07 b`` pixels.  A quad covers exactly one pixel centre and its four neighbours are background: every pixel of
    the band carries a coverage pair on both axes -- 128 per full 64-pixel chunk."""
    rng = np.random.default_rng(seed)
    jj, ii = np.meshgrid(np.arange(nj), np.arange(ni), indexing="ij")
    keep = (jj + ii) % 2 == 0
    jj, ii = jj[keep].astype(np.float64), ii[keep].astype(np.float64)
    pos = []
    for b in range(views):
        x0, y0 = i0 + ii + off[0] + 0.07 * b, j0 + jj + off[1] + 0.07 * b
        p, tri = S._quads(x0, y0, x0 + 1.0, y0 + 1.0, rng.uniform(-0.5, 0.5, len(ii)), H, W)
        pos.append(p)
    return np.stack(pos).astype(np.float32), tri.astype(np.int32)


def coverage(rast):
    """``[B, H, W]`` bool: the pixel shows a triangle."""
    return np.asarray(rast)[..., 3] > 0


def clamp_image(rast):
    """``clamp(rast[..., -1:], 0, 1)``: the colour image of the operators path, float32 0 / 1."""
    return np.clip(np.asarray(rast, dtype=np.float32)[..., 3:4], 0.0, 1.0)


def coverage_pairs(rast):
    """``c[B, H, W, 2]``: exactly one pixel of the pair (j, i) | right (axis 0) / upper (axis 1) neighbour is background."""
    cov = coverage(rast)
    c = np.zeros(cov.shape + (2,), dtype=bool)
    c[:, :, :-1, 0] = cov[:, :, 1:] != cov[:, :, :-1]
    c[:, :-1, :, 1] = cov[:, 1:, :] != cov[:, :-1, :]
    return c


def cover_masks(rast):
    """The coverage masks as tsamd_silhouette writes them: ``uint64[n_chunks, 2]``, bit l of word ``axis`` of chunk k = pixel
    64 k + l of the flattened batch has a coverage pair on that axis."""
    c = coverage_pairs(rast).reshape(-1, 2)
    n = (len(c) + 63) // 64
    c = np.concatenate([c, np.zeros((n * 64 - len(c), 2), dtype=bool)]).reshape(n, 64, 2)
    weights = np.uint64(1) << np.arange(64, dtype=np.uint64)
    return (c.astype(np.uint64) * weights[None, :, None]).sum(axis=1, dtype=np.uint64)


def split_events(events_b, cov_b):
    """(coverage events, foreground / foreground events) of one view."""
    cover = [ev for ev in events_b if cov_b[ev[0]] != cov_b[ev[1]]]
    both = [ev for ev in events_b if cov_b[ev[0]] and cov_b[ev[1]]]
    assert len(cover) + len(both) == len(events_b)                 # (a pair of two background pixels has no triangle)
    return cover, both


def events(rast, pos, tri, opp=None):
    """``(all events, coverage events)`` per view, from R.antialias_events."""
    cov = coverage(rast)
    ev = R.antialias_events(rast, pos, tri, opp)
    return ev, [split_events(ev[b], cov[b])[0] for b in range(len(ev))]


def silhouette(rast, pos, tri, opp=None, events=None):
    """``alpha[B, H, W, 1]`` float64 of the operators path."""
    return R.antialias(clamp_image(rast), rast, pos, tri, opp, events=events)


def silhouette_backward(rast, pos, tri, grad_alpha, opp=None, pos_gradient_boost=1.0, events=None):
    """``grad_pos[B, V, 4]`` float64 of the operators path."""
    return R.antialias_backward(clamp_image(rast), rast, pos, tri, grad_alpha, opp, pos_gradient_boost=pos_gradient_boost, events=events)[1]


def mse(alpha, target):
    """float64 mean squared error of two float32 images."""
    d = np.asarray(alpha, dtype=np.float32).astype(np.float64).reshape(-1) - np.asarray(target, dtype=np.float32).astype(np.float64).reshape(-1)
    return float(np.mean(d * d)) if d.size else 0.0


def mse_grad(alpha, target, upstream=1.0):
    """d (upstream * mse) / d alpha = 2 (alpha - target) upstream / n, float64, in the shape of ``alpha``."""
    a = np.asarray(alpha, dtype=np.float32).astype(np.float64)
    t = np.asarray(target, dtype=np.float32).astype(np.float64).reshape(a.shape)
    return 2.0 * (a - t) * float(upstream) / a.size


def gradient_terms(events_cov, pos, grad_alpha, res, boost):
    """Per ``grad_pos`` entry the number of terms and the sum of their absolute values (``count[B, V]``, ``mass[B, V, 4]``) over
    the coverage events, whose colour difference is 1: what the rounding-error bound of an fp32-atomic sum is made of."""
    H, W = res
    B, V = pos.shape[:2]
    mass, count = np.zeros((B, V, 4)), np.zeros((B, V))
    g = np.abs(np.asarray(grad_alpha, dtype=np.float64)).reshape(B, H, W)
    p64 = np.asarray(pos, dtype=np.float32).astype(np.float64)
    for b in range(B):
        for dst, _, _, _, _, (va, vb), (dA, dB) in events_cov[b]:
            a = abs(boost) * g[b][dst]
            for vtx, (ddx, ddy) in ((va, dA), (vb, dB)):
                x, y, _, w = p64[b, vtx]
                gx, gy = a * abs(ddx) * (0.5 * W / w), a * abs(ddy) * (0.5 * H / w)
                mass[b, vtx, 0] += gx
                mass[b, vtx, 1] += gy
                mass[b, vtx, 3] += (gx * abs(x) + gy * abs(y)) / w
                count[b, vtx] += 1
    return count, mass
