"""The argument checks the surface stages share (spheres_init, merge, metrics, simplify, voxelize): plain functions, one per thing
that can be wrong, which a module composes in its own order.  Every check names the function and the argument:
``tssplat_amd.<module>.<function>: <argument> must ...``.  ``fail`` is the module's ``functools.partial(_args.fail, "<module>")``.

What stays with a module: its ranges and wordings that no other module has, the order of its checks, and whether a tensor that is
not contiguous is copied or refused.  A new surface stage adds what it shares with the others here.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _capi

_GPU_ONLY = "must be a GPU tensor (there is no CPU fallback)"


def fail(module: str, name: str, what: str):
    raise RuntimeError(f"tssplat_amd.{module}.{name}: {what}")


def is_int(x, lo=-math.inf, hi=math.inf) -> bool:
    """A Python or numpy integer (a bool is not one) in ``lo .. hi``."""
    return not isinstance(x, bool) and isinstance(x, (int, np.integer)) and lo <= int(x) <= hi


def integer(fail, name: str, arg: str, x, lo: int, hi: int, hi_text=None) -> int:
    if not is_int(x, lo, hi):
        fail(name, f"{arg} must be an integer in {lo} .. {hi_text or hi}, got {x!r}")
    return int(x)


def bounds(fail, name: str, b, cells=None):
    """``(lo, hi)`` as floats: a pair, finite, ``lo < hi``, ``hi - lo`` finite and, with ``cells``, ``(hi - lo) / cells > 0``."""
    try:
        lo, hi = float(b[0]), float(b[1])
        two = len(b) == 2
    except (TypeError, ValueError, IndexError):
        lo = hi = math.nan
        two = False
    if not two or not (math.isfinite(lo) and math.isfinite(hi) and lo < hi and math.isfinite(hi - lo) and (cells is None or (hi - lo) / cells > 0.0)):
        fail(name, f"bounds must be (lo, hi), finite, with lo < hi, got {b!r}")
    return lo, hi


def choice(fail, name: str, arg: str, x, allowed) -> str:
    if not isinstance(x, str) or x not in allowed:
        fail(name, f"{arg} must be one of {', '.join(repr(a) for a in allowed)}, got {x!r}")
    return x


# ---- tensors: separate steps, so that a module says what it checks first ----
def dtype(fail, name: str, arg: str, t: torch.Tensor, want) -> None:
    if t.dtype != want:
        fail(name, f"{arg} must be {str(want).replace('torch.', '')}, got {str(t.dtype).replace('torch.', '')}")


def rows(fail, name: str, arg: str, t: torch.Tensor, cols: int, limit: int, shape: str) -> None:
    """``[N, cols]`` with ``N <= limit``; ``shape`` is how the module words that."""
    if t.dim() != 2 or t.shape[1] != cols or t.shape[0] > limit:
        fail(name, f"{arg} must be {shape}, got {tuple(t.shape)}")


def on_gpu(fail, name: str, arg: str, t) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        fail(name, f"{arg} {_GPU_ONLY}")


def on_device(fail, name: str, arg: str, t: torch.Tensor, device) -> None:
    if device is not None and t.device != device:
        fail(name, f"{arg} must live on the same device as the first tensor argument ({device}), got {t.device}")


def gpu_tensor(fail, name: str, arg: str, t, want, device=None) -> torch.Tensor:
    """Where it lives first (spheres_init, merge, metrics): on a GPU, of dtype ``want``, on ``device``.  Returns it detached."""
    on_gpu(fail, name, arg, t)
    dtype(fail, name, arg, t, want)
    on_device(fail, name, arg, t, device)
    return t.detach()


def typed_rows(fail, name: str, arg: str, t, want, limit: int) -> torch.Tensor:
    """What it is first (simplify, voxelize): a tensor of dtype ``want`` and shape ``[N, 3]`` with ``N <= limit``, wherever it lives."""
    if not isinstance(t, torch.Tensor):
        fail(name, f"{arg} {_GPU_ONLY}, got {type(t).__name__}")
    dtype(fail, name, arg, t, want)
    rows(fail, name, arg, t, 3, limit, f"[N, 3] with N <= {limit}")
    return t


def placed(fail, name: str, arg: str, t: torch.Tensor, device=None) -> torch.Tensor:
    """The second half of ``typed_rows``: on a GPU, on ``device``.  Returns it detached."""
    on_gpu(fail, name, arg, t)
    on_device(fail, name, arg, t, device)
    return t.detach()


def triangle_mesh(fail, name: str, v, faces, max_faces: int, v_arg: str = "v", f_arg: str = "faces", device=None):
    """float32 ``[N, 3]`` vertices and int32 ``[N, 3]`` faces: types and shapes of both first, then where they live -- what is wrong
    with an argument is said before where it is.  Returns both detached."""
    v = typed_rows(fail, name, v_arg, v, torch.float32, 2 ** 31 - 1)
    faces = typed_rows(fail, name, f_arg, faces, torch.int32, max_faces)
    v = placed(fail, name, v_arg, v, device)
    return v, placed(fail, name, f_arg, faces, v.device)


# ---- the way into the library ----
def ptr(t: torch.Tensor):
    """The device pointer, or null for an empty tensor (the C entry points take null where there is nothing to read or write)."""
    return t.data_ptr() if t.numel() else None


def lib_and_stream(device):
    from .tet_spheres_ext import _device_ctx, _stream_ptr
    return _capi.load(), _device_ctx(device), _stream_ptr(device)
