"""Float64 statements of the streaming step operations of include/tssplat_amd.h -- TEST INFRASTRUCTURE.

``scale``, ``grad_limit`` and ``adam_step`` restate the formulae in the header comments of ``tsamd_scale``,
``tsamd_grad_limit`` and ``tsamd_adam_uniform_step`` on float64 copies of fp32 inputs; scalars are used as given (the GPU
tests pass values already rounded to fp32, because the ABI takes ``float``).  Written from the header, not from the kernels.

Per-entry error bounds of an fp32 implementation, ``U = 2^-24``: the number of fp32 roundings in the operation chain plus one.

* ``scale``: one multiply -- compared bit for bit with ``np.float32(x) * np.float32(s)``, no bound.
* ``grad_limit``: a clamped entry is one correctly rounded divide and one multiply, ``3 U |ref|``; an unclamped entry is the
  input, bit for bit.
* Adam moments: ``6 U (|g1 b1| + |grad (1 - b1)|)`` and ``6 U (|g2 b2| + |grad^2 (1 - b2)|)`` -- at most 5 roundings each,
  whether or not the compiler contracts the multiply-adds.
* Adam parameter: ``2^-23 |p_ref| + 32 U |lr gr_ref|`` -- the step factor passes through about 10 roundings unclamped and
  about 24 clamped (the two maxima, their bias corrections, the square root, the reciprocal, the clamp ratio), the moment
  adds its 4 and the final multiply-add half an ulp of ``p``.

``emulate_*`` are fp32 numpy emulations of the same formulae (separately rounded, or with the multiply-adds fused) whose
maxima can be told to overlook entries: tests/test_step_kernels.py shows with them, without a GPU, that a correct fp32
implementation stays inside the bounds and that one whose maximum misses a region does not.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _absmax(a, mask=None):
    """max |a| over the entries the mask keeps; 0 for none (the maxima of the step start from 0)."""
    a = np.abs(a) if mask is None else np.abs(a[mask])
    return float(a.max()) if a.size else 0.0


def scale(x, s):
    """out = in * scalar."""
    return _f64(x) * float(s)


def grad_limit(g, thr, s, mask=None):
    """if max|g| > thr: g *= s / max|g|.  Returns (result, clamped).  ``mask``: entries the maximum is taken over."""
    g = _f64(g)
    m = _absmax(g, mask)
    if m > thr:
        with np.errstate(invalid="ignore", divide="ignore"):
            return g * (float(s) / m), True
    return g.copy(), False


def grad_limit_bound(ref):
    return 3 * U * np.abs(ref)


def adam_step(p, grad, g1, g2, lr, b1, b2, step, limit, mask=None):
    """One AdamUniform step from a given state (tsamd_adam_uniform_step's header comment):
        g1 = b1 g1 + (1-b1) grad;  g2 = b2 g2 + (1-b2) grad^2
        gr = (g1 / (1-b1^step)) / (1e-8 + max sqrt(g2 / (1-b2^step)))
        if limit > 0 and max|gr| > limit: gr *= limit / max|gr|
        p -= lr gr
    ``mask`` (boolean, optional): the entries both maxima are taken over.  Returns p, g1, g2, gr and the magnitudes
    mag1 = |g1 b1| + |grad (1-b1)|, mag2 = |g2 b2| + |grad^2 (1-b2)| the bounds need, and whether the clamp acted."""
    p, grad, g1, g2 = _f64(p), _f64(grad), _f64(g1), _f64(g2)
    lr, b1, b2, limit = float(lr), float(b1), float(b2), float(limit)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        a1, c1 = g1 * b1, grad * (1 - b1)
        a2, c2 = g2 * b2, grad * grad * (1 - b2)
        n1, n2 = a1 + c1, a2 + c2
        m1 = n1 / (1 - b1 ** step)
        m2 = n2 / (1 - b2 ** step)
        gr = m1 / (1e-8 + _absmax(np.sqrt(m2), mask))
        clamped = False
        if limit > 0:
            s = _absmax(gr, mask)
            if s > limit:
                gr = gr * (limit / s)
                clamped = True
        return SimpleNamespace(p=p - lr * gr, g1=n1, g2=n2, gr=gr, mag1=np.abs(a1) + np.abs(c1), mag2=np.abs(a2) + np.abs(c2),
                               clamped=clamped)


def moment_bound(mag):
    return 6 * U * mag


def param_bound(ref, lr):
    return 2.0 ** -23 * np.abs(ref.p) + 32 * U * np.abs(float(lr) * ref.gr)


# ---- fp32 emulations ----------------------------------------------------------------------------------------------------------

_f = np.float32


def _fma(a, b, c):
    """a * b + c with the product unrounded (exact in float64: 24 + 24 bits), the sum rounded to fp32."""
    return (a.astype(np.float64) * np.float64(b) + np.asarray(c, dtype=np.float64)).astype(np.float32)


def emulate_scale(x, s):
    return np.asarray(x, dtype=np.float32) * _f(s)


def emulate_grad_limit(g, thr, s, seen=None):
    """fp32 clamp; ``seen``: the entries the maximum looks at (None = all; NaN never wins a maximum, as with fmaxf)."""
    g = np.asarray(g, dtype=np.float32)
    m = _f(np.fmax.reduce(np.abs(g if seen is None else g[seen]), initial=_f(0)))
    if not m > _f(thr):
        return g.copy()
    with np.errstate(invalid="ignore", divide="ignore"):
        return g * (_f(s) / m)


def emulate_adam_step(p, grad, g1, g2, lr, b1, b2, step, limit, fused=False, seen=None):
    """fp32 AdamUniform step with every operation rounded on its own, or (``fused``) with the multiply-adds fused.
    ``seen``: the entries the two maxima look at (None = all).  Returns (p, g1, g2)."""
    p, grad, g1, g2 = (np.asarray(a, dtype=np.float32) for a in (p, grad, g1, g2))
    lr, b1, b2, limit = _f(lr), _f(b1), _f(b2), _f(limit)
    one = _f(1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if fused:
            n1 = _fma(g1, b1, grad * (one - b1))
            n2 = _fma(g2, b2, (grad * grad) * (one - b2))
        else:
            n1 = g1 * b1 + grad * (one - b1)
            n2 = g2 * b2 + (grad * grad) * (one - b2)
        bias1 = _f(1.0 - float(b1) ** step)
        bias2 = _f(1.0 - float(b2) ** step)
        mx1 = _f(np.fmax.reduce(np.abs(n1 if seen is None else n1[seen]), initial=_f(0))) / bias1
        mx2 = _f(np.fmax.reduce(n2 if seen is None else n2[seen], initial=_f(0)))
        denom = _f(1e-8) + np.sqrt(mx2 / bias2)
        sc = one / denom
        s = mx1 / denom
        if limit > 0 and s > limit:
            sc = sc * (limit / s)
        k = lr * sc / bias1
        q = _fma(n1, -k, p) if fused else p - k * n1
    return q, n1, n2
