"""The float32 statement of the rasteriser's VALUE path (tssplat_amd/csrc/raster_kernels.hip, interpolate_kernels.hip and
the helpers they share, raster_device.h): numpy, every operation rounded to ``np.float32`` on its own, in the kernel's order -- TEST
INFRASTRUCTURE.

Coverage and depth stay defined by ``oracle/raster_oracle.py::rasterize_ids`` (integers and a float32 depth plane, already bit for
bit); this module takes its winning ids and restates what the kernels compute from them:

    edge_functions          the homogeneous edge functions of a pixel centre (the ONE statement every kernel shares)
    resolve32               rasterize_resolve_kernel: (u, v, z/w, id + 1)
    interpolate32           interpolate_kernel
    interpolate_backward32  interpolate_backward_kernel: grad_rast per pixel and the per-pixel scatter terms of grad_attr
    rasterize_backward32    rasterize_backward_kernel: the nine per-pixel contributions of edge_functions_backward

The kernel files are compiled without contraction and float32 division is correctly rounded, so a numpy float32 array operation
(one IEEE operation, round to nearest even) is the same function of the same bits: the results must agree with the device BIT FOR
BIT.  The one place where C leaves a choice is the sign of ``fmaxf(-0, +0)`` in the clamp of a barycentric that is exactly ``-0``:
gfx9's ``v_max_f32`` / ``v_med3_f32`` order -0 below +0 (IEEE 754-2019 ``maximumNumber``), so the clamp gives +0, and that is what is
stated here.  ``resolve32`` also names those pixels (``zero_sign``) from its own pre-clamp values, so that a test can count them and,
if it has to, compare them by value instead of by bits.
"""
from __future__ import annotations

import numpy as np

from oracle import raster_oracle as R

f32 = np.float32
U = 2.0 ** -24                                   # unit roundoff of float32
_0, _1, _2, _H = f32(0.0), f32(1.0), f32(2.0), f32(0.5)


def _f(x):
    return np.asarray(x, dtype=np.float32)


def edge_functions(v0, v1, v2, px, py, H, W):
    """``EdgeFunctions`` of the kernel for arrays of pixels: ``v_k[n, 4]`` float32 clip-space vertices, ``px, py[n]`` integers.
    Returns a dict of float32 arrays (fx, fy, p0x .. p2y, a0, a1, a2, s with ``s == 0 -> 1``)."""
    v0, v1, v2 = _f(v0), _f(v1), _f(v2)
    e = {}
    e["fx"] = (_f(px) + _H) / f32(W) * _2 - _1
    e["fy"] = (_f(py) + _H) / f32(H) * _2 - _1
    for k, v in enumerate((v0, v1, v2)):
        e[f"p{k}x"] = v[:, 0] - e["fx"] * v[:, 3]
        e[f"p{k}y"] = v[:, 1] - e["fy"] * v[:, 3]
    e["a0"] = e["p1x"] * e["p2y"] - e["p1y"] * e["p2x"]
    e["a1"] = e["p2x"] * e["p0y"] - e["p2y"] * e["p0x"]
    e["a2"] = e["p0x"] * e["p1y"] - e["p0y"] * e["p1x"]
    s = e["a0"] + e["a1"] + e["a2"]
    e["s"] = np.where(s == _0, _1, s)
    assert all(a.dtype == np.float32 for a in e.values())
    return e


def _clamp(x, lo, hi):
    """``fminf(fmaxf(x, lo), hi)``: a NaN gives ``lo``; ``fmaxf(-0, +0)`` is +0 (the device orders the zeros)."""
    y = np.fmin(np.fmax(x, f32(lo)), f32(hi))
    return np.where(y == _0, _0, y) if lo == 0 else y


def ids_of(key):
    """Triangle id per pixel (-1 on background) of a key image of ``rasterize_ids``."""
    return np.where(key == R.NO_FRAGMENT, -1, (key & np.uint64(0xFFFFFFFF)).astype(np.int64))


def resolve32(pos_clip, tri, keys):
    """``rast[B, H, W, 4]`` float32 as the resolve pass writes it, from ``keys[B, H, W]`` (``rasterize_ids`` per view), and
    ``zero_sign[B, H, W]``: pixels where a barycentric is exactly -0 before the clamp (the sign of the clamped zero is open)."""
    pos = _f(pos_clip)
    pos = pos[None] if pos.ndim == 2 else pos
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    keys = np.asarray(keys)
    keys = keys[None] if keys.ndim == 2 else keys
    B, H, W = keys.shape
    out = np.zeros((B, H, W, 4), dtype=np.float32)
    zero_sign = np.zeros((B, H, W), dtype=bool)
    with np.errstate(all="ignore"):
        for b in range(B):
            ids = ids_of(keys[b])
            jj, ii = np.nonzero(ids >= 0)
            if not len(jj):
                continue
            t = ids[jj, ii]
            v0, v1, v2 = (pos[b][tri[t, k]] for k in range(3))
            e = edge_functions(v0, v1, v2, ii, jj, H, W)
            b0, b1 = e["a0"] / e["s"], e["a1"] / e["s"]
            b2 = (_1 - b0) - b1
            z = (b0 * v0[:, 2] + b1 * v1[:, 2]) + b2 * v2[:, 2]
            w = (b0 * v0[:, 3] + b1 * v1[:, 3]) + b2 * v2[:, 3]
            w = np.where(w == _0, _1, w)
            out[b, jj, ii, 0] = _clamp(b0, 0, 1)
            out[b, jj, ii, 1] = _clamp(b1, 0, 1)
            out[b, jj, ii, 2] = _clamp(z / w, -1, 1)
            out[b, jj, ii, 3] = (t + 1).astype(np.float32)
            zero_sign[b, jj, ii] = ((b0 == _0) & np.signbit(b0)) | ((b1 == _0) & np.signbit(b1))
    return out, zero_sign


def rasterize32(pos_clip, tri, resolution):
    """``(rast, zero_sign, keys)`` of a batch: the oracle's coverage, this module's values."""
    pos = _f(pos_clip)
    pos = pos[None] if pos.ndim == 2 else pos
    H, W = int(resolution[0]), int(resolution[1])
    keys = np.stack([R.rasterize_ids(pos[b], tri, H, W) for b in range(pos.shape[0])])
    rast, zero_sign = resolve32(pos, tri, keys)
    return rast, zero_sign, keys


def same_bits(got, want, zero_sign=None):
    """``np.array_equal`` on the raw float32 bits; where ``zero_sign`` is set, -0 and +0 of the first two channels count as equal."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return False
    g, w = got.view(np.uint32).copy(), want.view(np.uint32).copy()
    if zero_sign is not None and zero_sign.any():
        for c in (0, 1):
            both_zero = zero_sign & (got[..., c] == 0) & (want[..., c] == 0)
            g[..., c][both_zero] = 0
            w[..., c][both_zero] = 0
    return np.array_equal(g, w)


def triangle_of(w, tri, n_vertices):
    """``triangle_of`` + ``triangle_indices`` of the kernel: the triangle a rast pixel's fourth channel names, -1 for background,
    a non-finite value, an id outside ``[0, n_tri)`` or a triangle with a vertex index outside ``[0, n_vertices)``."""
    w = _f(w)
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        ok = (w >= _1) & (w <= f32(16777216.0))
    t = np.where(ok, w, _1).astype(np.int64) - 1
    ok &= t < len(tri)
    t = np.where(ok, t, 0)
    if len(tri):
        ok &= np.all((tri[t] >= 0) & (tri[t] < n_vertices), axis=-1)
    return np.where(ok, t, -1)


def _gather_attr(attr, rast, tri):
    attr, rast = _f(attr), _f(rast)
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    t = triangle_of(rast[..., 3], tri, attr.shape[1])
    hit = t >= 0
    bb = np.nonzero(hit)[0]
    ab = bb if attr.shape[0] > 1 else np.zeros_like(bb)
    tt = tri[t[hit]] if len(tri) else np.zeros((0, 3), dtype=np.int64)
    a = [attr[ab, tt[:, k]] for k in range(3)]
    u, v = rast[..., 0][hit], rast[..., 1][hit]
    w = (_1 - u) - v
    return hit, ab, tt, a, u, v, w


def interpolate32(attr, rast, tri):
    """``interpolate_kernel``: ``(u a0 + v a1) + w a2`` with ``w = (1 - u) - v`` from ``rast``'s own bits; 0 on background."""
    with np.errstate(all="ignore"):
        hit, _, _, a, u, v, w = _gather_attr(attr, rast, tri)
        out = np.zeros(np.shape(rast)[:3] + (np.shape(attr)[-1],), dtype=np.float32)
        out[hit] = (u[:, None] * a[0] + v[:, None] * a[1]) + w[:, None] * a[2]
    return out


def interpolate_backward32(attr, rast, tri, grad_out):
    """``interpolate_backward_kernel`` per pixel: ``grad_rast[B, H, W, 4]`` (du, dv accumulated over the channels in order, from
    0) and the scatter terms -- ``(hit[B, H, W], attr_batch[n], vertices[n, 3], terms[n, 3, C])`` with ``terms[:, k]`` the float32
    products ``(u, v, w)[k] * g`` a valid pixel adds to vertex ``k`` of its triangle."""
    g = _f(grad_out)
    with np.errstate(all="ignore"):
        hit, ab, tt, a, u, v, w = _gather_attr(attr, rast, tri)
        gg = g[hit]
        du = np.zeros(len(u), dtype=np.float32)
        dv = np.zeros(len(u), dtype=np.float32)
        for c in range(g.shape[-1]):
            du = du + gg[:, c] * (a[0][:, c] - a[2][:, c])
            dv = dv + gg[:, c] * (a[1][:, c] - a[2][:, c])
        grad_rast = np.zeros(np.shape(rast), dtype=np.float32)
        grad_rast[..., 0][hit] = du
        grad_rast[..., 1][hit] = dv
        terms = np.stack([u[:, None] * gg, v[:, None] * gg, w[:, None] * gg], axis=1)
    assert terms.dtype == np.float32
    return grad_rast, (hit, ab, tt, terms)


def rasterize_backward32(pos_clip, tri, rast, grad_rast):
    """``rasterize_backward_kernel`` per pixel: ``(view[n], vertices[n, 3], d[n, 9])`` with ``d[:, 3 k ..]`` the float32
    contributions to (x, y, w) of vertex ``k``, operation by operation as ``edge_functions_backward``; pixels with
    ``g.x == g.y == 0``, background and ids outside the list contribute nothing."""
    pos, rast, g = _f(pos_clip), _f(rast), _f(grad_rast)
    pos = pos[None] if pos.ndim == 2 else pos
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    B, H, W = rast.shape[:3]
    t = rast[..., 3].astype(np.int64) - 1
    ok = (t >= 0) & (t < len(tri)) & ~((g[..., 0] == _0) & (g[..., 1] == _0))
    if len(tri):
        tv = tri[np.where(ok, t, 0)]
        ok &= np.all((tv >= 0) & (tv < pos.shape[1]), axis=-1)
    bb, jj, ii = np.nonzero(ok)
    tt = tri[t[ok]] if len(tri) else np.zeros((0, 3), dtype=np.int64)
    with np.errstate(all="ignore"):
        e = edge_functions(pos[bb, tt[:, 0]], pos[bb, tt[:, 1]], pos[bb, tt[:, 2]], ii, jj, H, W)
        gu, gv = g[..., 0][ok], g[..., 1][ok]
        inv = _1 / e["s"]
        u, v = e["a0"] * inv, e["a1"] * inv
        dot = gu * u + gv * v
        da0, da1, da2 = (gu - dot) * inv, (gv - dot) * inv, -dot * inv
        d = np.zeros((len(bb), 9), dtype=np.float32)
        d[:, 0], d[:, 1] = da1 * -e["p2y"] + da2 * e["p1y"], da1 * e["p2x"] + da2 * -e["p1x"]
        d[:, 3], d[:, 4] = da0 * e["p2y"] + da2 * -e["p0y"], da0 * -e["p2x"] + da2 * e["p0x"]
        d[:, 6], d[:, 7] = da0 * -e["p1y"] + da1 * e["p0y"], da0 * e["p1x"] + da1 * -e["p0x"]
        for k in range(3):
            d[:, 3 * k + 2] = -e["fx"] * d[:, 3 * k] - e["fy"] * d[:, 3 * k + 1]
    return bb, tt, d


def any_order_sum_check(got, index, terms, shape):
    """The any-order summation bound: ``|got - sum_i c_i| <= gamma_(n-1) sum_i |c_i|`` per entry, ``gamma_k = k U / (1 - k U)``,
    ``n`` the number of terms of the entry (``terms[i]`` goes to flat entry ``index[i]`` of an array of ``shape``; float32 terms,
    summed here in float64).  Returns ``(ok, max error / bound, exact_zero_ok)``: entries without a term must be exactly 0."""
    size = int(np.prod(shape))
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    terms = np.asarray(terms, dtype=np.float64)
    total, mass = np.zeros(size), np.zeros(size)
    count = np.zeros(size, dtype=np.int64)
    np.add.at(total, index, terms)
    np.add.at(mass, index, np.abs(terms))
    np.add.at(count, index, 1)
    k = np.maximum(count - 1, 0) * U
    bound = k / (1.0 - k) * mass
    err = np.abs(got - total)
    zero_ok = bool(np.all(got[count == 0] == 0.0))
    some = (count > 1) & (bound > 0)
    ratio = float(np.max(err[some] / bound[some])) if some.any() else 0.0
    return bool(np.all(err <= bound)), ratio, zero_ok


def scatter_index(view, vertices, n_vertices, width, columns):
    """Flat entries ``((view * n_vertices + vertex) * width + column)`` for ``vertices[n, 3]`` x ``columns``: ``[n, 3, len(columns)]``."""
    base = (np.asarray(view)[:, None] * n_vertices + vertices) * width
    return base[:, :, None] + np.asarray(columns)[None, None, :]
