"""Oracle of the normal term (dr.silhouette_normal_mse, tsamd_normal_mse*): numpy only, float64, composed of oracle/raster_oracle.py.

The specification is the operator chain of MeshRasterizer.forward(fit_normal=True) under a masked MSELoss, for any 3-channel vertex
attribute ``attr[V, 3]`` (the renderer passes the vertex normals times [1, 1, -1]):

    n    = interpolate(attr[None], rast, tri)                 R.interpolate; 0 on background
    loss = mean((n_c m - t_c m)^2)                            over B H W 3 values, the mask m[B, H, W] broadcast over the channels

and backwards ``g_c = upstream 2 (n_c m - t_c m) m / (3 B H W)``, R.interpolate_backward (the scatter into ``grad_attr`` and
``(du, dv)``), R.rasterize_backward (``grad_pos``; the clamps of (u, v) treated as inactive).

Two rounding bounds of the float32 kernels follow, each derived where it is stated; ``U = 2^-24`` is the unit round-off.
"""
from __future__ import annotations

import numpy as np

from depth_oracle import U, _known_ids
from oracle import raster_oracle as R


def _attr(attr):
    return np.asarray(attr, dtype=np.float64).reshape(1, -1, 3)


def _mask(mask, shape):
    return np.asarray(mask, dtype=np.float64).reshape(shape[:3] + (1,))


def normals(rast, tri, attr):
    """``n[B, H, W, 3]`` float64 of the chain: the interpolated attribute, 0 on background."""
    return R.interpolate(_attr(attr), rast, tri)


def loss64(n, target, mask):
    """``mean((n m - t m)^2)`` in float64 of float32 images (0 of nothing)."""
    n = np.asarray(n, dtype=np.float64)
    m = _mask(mask, n.shape)
    x = n * m - np.asarray(target, dtype=np.float64).reshape(n.shape) * m
    return float(np.mean(x * x)) if x.size else 0.0


def loss(rast, tri, attr, target, mask):
    return loss64(normals(rast, tri, attr), target, mask)


def backward(rast, pos, tri, attr, target, mask, upstream=1.0):
    """``(grad_attr[V, 3], grad_pos[B, V, 4])`` float64 of ``upstream * loss``."""
    rast = np.asarray(rast, dtype=np.float64)
    attr1 = _attr(attr)
    n = R.interpolate(attr1, rast, tri)
    m = _mask(mask, n.shape)
    t = np.asarray(target, dtype=np.float64).reshape(n.shape)
    g = float(upstream) * 2.0 * (n * m - t * m) * m / n.size
    grad_attr, grad_rast = R.interpolate_backward(attr1, rast, tri, g)
    grad_pos = R.rasterize_backward(pos, tri, _known_ids(rast, tri, attr1.shape[1]), grad_rast)
    return grad_attr[0], grad_pos


def normal_bound(rast32, tri, attr):
    """``(n64, bound)``, both ``[B, H, W, 3]``, with ``|n_gpu - n64| <= bound = 4.5 U (|u a0| + |v a1| + |w a2|)`` per component.

    ``n64`` is evaluated in float64 from the kernel's own float32 weights: ``(u, v)`` of ``rast32`` (the kernel forms them by the
    operations of the resolve pass, so they are these bits) and ``w = fl(fl(1 - u) - v)`` formed in float32 here.  From there on the
    kernel rounds ``n_c = fl(fl(fl(u a0) + fl(v a1)) + fl(w a2))``: the terms ``u a0`` and ``v a1`` pass through three roundings
    each (their product and the two sums), ``w a2`` through two, and the error of a sum's rounding is relative to a partial sum
    that the absolute values of its terms bound, so ``|n_c - n64_c| <= 3 U (|u a0| + |v a1| + |w a2|)`` to first order.  ``4.5``
    leaves the second-order terms and the error of ``n64``'s own float64 evaluation (~2^-52 of the same sum) half as much again as
    the first-order terms need -- the headroom depth_oracle.depth_bound gives its own (4 -> 6).  On background both are 0."""
    rast32 = np.asarray(rast32, dtype=np.float32)
    B, H, W = rast32.shape[:3]
    attr = np.asarray(attr, dtype=np.float64).reshape(-1, 3)
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    n64 = np.empty((B, H, W, 3))
    bound = np.empty((B, H, W, 3))
    for b in range(B):
        ids, hit = R._valid_ids(rast32[b, ..., 3].astype(np.float64), tri, attr.shape[0])
        u32, v32 = rast32[b, ..., 0], rast32[b, ..., 1]
        w32 = (np.float32(1.0) - u32) - v32                       # float32 arithmetic: two roundings
        u, v, w = (np.where(hit, k.astype(np.float64), 0.0)[..., None] for k in (u32, v32, w32))
        t = tri[np.where(hit, ids, 0)]
        a0, a1, a2 = attr[t[..., 0]], attr[t[..., 1]], attr[t[..., 2]]
        n64[b] = u * a0 + v * a1 + w * a2
        bound[b] = 4.5 * U * (np.abs(u * a0) + np.abs(v * a1) + np.abs(w * a2))
    return n64, bound


def loss_bound(n_gpu, target, mask):
    """``(loss64, bound)`` with ``|loss_gpu - loss64(n_gpu)| <= bound = mean(2 |x| g (|n m| + |t m| + |x|)) + 2 g loss64``,
    ``g = 1.01 U``, ``x = n m - t m`` in float64 of the kernel's own float32 ``n``, the mean over ``B H W 3`` values.

    depth_oracle.loss_bound over three channels: per channel the kernel forms ``r = fl(fl(n m) - fl(t m)) = x + e`` with
    ``|e| <= U |n m| + U |t m| + U |x|`` to first order (the factor 1.01 takes the second-order terms), squares and adds in float64
    (errors ~2^-53 per operation: nothing at this scale), so each square is off by ``|r^2 - x^2| <= 2 |x| |e| + e^2``; ``e^2`` and
    the rounding of the mean to float32 (``U loss``) are inside ``2 g loss64``."""
    n = np.asarray(n_gpu, dtype=np.float32).astype(np.float64)
    m = _mask(mask, n.shape)
    t = np.asarray(target, dtype=np.float64).reshape(n.shape)
    x = n * m - t * m
    want = float(np.mean(x * x)) if x.size else 0.0
    g = 1.01 * U
    bound = (float(np.mean(2.0 * np.abs(x) * g * (np.abs(n * m) + np.abs(t * m) + np.abs(x)))) if x.size else 0.0) + 2.0 * g * want
    return want, bound
