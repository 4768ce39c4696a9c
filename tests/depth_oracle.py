"""Oracle of the depth term (dr.silhouette_depth_mse, tsamd_depth_mse*): numpy only, float64, composed of oracle/raster_oracle.py.

The specification is the operator chain of MeshRasterizer.forward(fit_depth=True) and trainer.py's depth loss:

    x    = interpolate(world_pos[None], rast, tri)            R.interpolate
    d    = || x - campos[:, None, None, :] ||                 (|| campos || on background, where x = 0)
    loss = mean((d m - t m)^2)                                over B H W pixels

and backwards ``g_d = upstream 2 (d m - t m) m / n``, ``g_x = g_d (x - campos) / d`` (0 where d = 0), R.interpolate_backward
(the scatter into ``grad_world`` and ``(du, dv)``), R.rasterize_backward (``grad_pos``; the clamps of (u, v) treated as inactive).

Two rounding bounds of the float32 kernels follow, each derived where it is stated; ``U = 2^-24`` is the unit round-off.
"""
from __future__ import annotations

import numpy as np

from oracle import raster_oracle as R

U = 2.0 ** -24


def _camera(campos, B):
    c = np.asarray(campos, dtype=np.float64).reshape(B, 3)
    return c[:, None, None, :]


def _image(a, shape):
    return np.asarray(a, dtype=np.float64).reshape(shape)


def positions(rast, tri, world):
    """``x[B, H, W, 3]`` float64: the interpolated world positions, 0 on background."""
    world = np.asarray(world, dtype=np.float64).reshape(1, -1, 3)
    return R.interpolate(world, rast, tri)


def depth(rast, tri, world, campos):
    """``d[B, H, W]`` float64 of the chain."""
    x = positions(rast, tri, world)
    return np.linalg.norm(x - _camera(campos, x.shape[0]), axis=-1)


def loss64(d, target, mask):
    """``mean((d m - t m)^2)`` in float64 of float32 images (0 of nothing)."""
    d = np.asarray(d, dtype=np.float64)
    x = d * _image(mask, d.shape) - _image(target, d.shape) * _image(mask, d.shape)
    return float(np.mean(x * x)) if x.size else 0.0


def loss(rast, tri, world, campos, target, mask):
    return loss64(depth(rast, tri, world, campos).reshape(np.asarray(rast).shape[:3]), target, mask)


def backward(rast, pos, tri, world, campos, target, mask, upstream=1.0):
    """``(grad_world[V, 3], grad_pos[B, V, 4])`` float64 of ``upstream * loss``."""
    rast = np.asarray(rast, dtype=np.float64)
    B, H, W = rast.shape[:3]
    world1 = np.asarray(world, dtype=np.float64).reshape(1, -1, 3)
    x = R.interpolate(world1, rast, tri)
    delta = x - _camera(campos, B)
    d = np.linalg.norm(delta, axis=-1)
    m, t = _image(mask, d.shape), _image(target, d.shape)
    g_d = float(upstream) * 2.0 * (d * m - t * m) * m / d.size
    with np.errstate(divide="ignore", invalid="ignore"):
        g_x = np.where(d[..., None] == 0.0, 0.0, g_d[..., None] * delta / np.where(d == 0.0, 1.0, d)[..., None])
    grad_attr, grad_rast = R.interpolate_backward(world1, rast, tri, g_x)
    grad_pos = R.rasterize_backward(pos, tri, _known_ids(rast, tri, world1.shape[1]), grad_rast)
    return grad_attr[0], grad_pos


def _known_ids(rast, tri, n_vertices):
    """``rast`` with the id channel of the pixels ``interpolate`` treats as background set to 0 (R.rasterize_backward indexes the
    triangle list with whatever the channel holds)."""
    out = np.array(rast, dtype=np.float64)
    for b in range(out.shape[0]):
        _, hit = R._valid_ids(out[b, ..., 3], np.asarray(tri, dtype=np.int64).reshape(-1, 3), n_vertices)
        out[b, ..., 3][~hit] = 0.0
    return out


def depth_bound(rast32, tri, world, campos):
    """``(d64, bound)`` with ``|d_gpu - d64| <= bound = U (6 S + 4 d64)`` per pixel.

    ``d64`` is evaluated in float64 from the kernel's own float32 weights: ``(u, v)`` of ``rast32`` (the kernel forms them by the
    operations of the resolve pass, so they are these bits) and ``w = fl(fl(1 - u) - v)`` formed in float32 here.  From there on the
    kernel rounds: per component ``x_c = fl(fl(fl(u a0) + fl(v a1)) + fl(w a2))`` -- every term passes through at most three
    roundings, so ``|x_c - x64_c| <= 3 U (|u a0| + |v a1| + |w a2|)`` to first order -- and ``delta_c = fl(x_c - c_c)`` adds
    ``U |delta_c| <= U (|u a0| + |v a1| + |w a2| + |c_c|)``: ``|delta_c - delta64_c| <= 4 U S_c`` with
    ``S_c = |u| |a0_c| + |v| |a1_c| + |w| |a2_c| + |c_c|``.  The norm is 1-Lipschitz: these errors move d by at most
    ``4 U ||S||_2``.  The norm itself: three squares (U each), two additions (2 U on the sum), together a relative 3 U on the sum of
    squares = 1.5 U on its root, and a square root within one ulp (2 U): ``3.5 U d``.  ``6 S`` and ``4 d`` leave the second-order
    terms and the error of ``d64``'s own float64 evaluation (~2^-50) half as much again as the first-order terms need."""
    rast32 = np.asarray(rast32, dtype=np.float32)
    B, H, W = rast32.shape[:3]
    world = np.asarray(world, dtype=np.float64).reshape(-1, 3)
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    c = np.asarray(campos, dtype=np.float64).reshape(B, 3)
    d64 = np.empty((B, H, W))
    bound = np.empty((B, H, W))
    for b in range(B):
        ids, hit = R._valid_ids(rast32[b, ..., 3].astype(np.float64), tri, world.shape[0])
        u32, v32 = rast32[b, ..., 0], rast32[b, ..., 1]
        w32 = (np.float32(1.0) - u32) - v32                       # float32 arithmetic: two roundings
        u, v, w = (np.where(hit, k.astype(np.float64), 0.0)[..., None] for k in (u32, v32, w32))
        t = tri[np.where(hit, ids, 0)]
        a0, a1, a2 = world[t[..., 0]], world[t[..., 1]], world[t[..., 2]]
        x = u * a0 + v * a1 + w * a2
        S = np.abs(u) * np.abs(a0) + np.abs(v) * np.abs(a1) + np.abs(w) * np.abs(a2) + np.abs(c[b])
        d64[b] = np.linalg.norm(x - c[b], axis=-1)
        bound[b] = U * (6.0 * np.linalg.norm(S, axis=-1) + 4.0 * d64[b])
    return d64, bound


def loss_bound(d_gpu, target, mask):
    """``(loss64, bound)`` with ``|loss_gpu - loss64(d_gpu)| <= bound = mean(2 |x| g (|d m| + |t m| + |x|)) + 2 g loss64``,
    ``g = 1.01 U``, ``x = d m - t m`` in float64 of the kernel's own float32 ``d``.

    The kernel forms ``r = fl(fl(d m) - fl(t m)) = x + e`` with ``|e| <= U |d m| + U |t m| + U |x|`` to first order (the factor 1.01
    takes the second-order terms), squares and adds in float64 (errors ~2^-53 per operation: nothing at this scale), so each
    square is off by ``|r^2 - x^2| <= 2 |x| |e| + e^2``; ``e^2`` and the rounding of the mean to float32 (``U loss``) are inside
    ``2 g loss64``."""
    d = np.asarray(d_gpu, dtype=np.float32).astype(np.float64)
    m, t = _image(mask, d.shape), _image(target, d.shape)
    x = d * m - t * m
    want = float(np.mean(x * x)) if x.size else 0.0
    g = 1.01 * U
    bound = (float(np.mean(2.0 * np.abs(x) * g * (np.abs(d * m) + np.abs(t * m) + np.abs(x)))) if x.size else 0.0) + 2.0 * g * want
    return want, bound
