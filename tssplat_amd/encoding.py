"""Multiresolution hash-grid encoding on the gfx950 kernels (csrc/grid_kernels.hip): the colour field's input encoding of the
texture stage (/root/reference/materials/explicit_material.py, models/networks.py:97-106, ``tcnn.Encoding``).

Semantics: tiny-cuda-nn's ``Grid`` encoding (Instant-NGP, Mueller et al. 2022) as tests/hashgrid_oracle.py restates it --
PARITY UNPINNED against the library itself (CUDA only, not available here).  ``params`` holds the table in tiny-cuda-nn's
layout (level-major, ``n_features_per_level`` contiguous fp32 values per entry); the per-level layout comes from the library's
own host function (``tsamd_grid_layout``), so the Python and C layouts cannot drift apart.

Domain: finite ``x`` with ``|scale_l * x + 0.5| < 2^31`` on every level (``scale_l`` at most 65535).  Rows outside it (larger
positions, +-inf, NaN) have unspecified values -- their outputs, their dL/dx and what they add to dL/dparams; every table
index is still reduced modulo the level's entry count, so all accesses stay in bounds, and the outputs and dL/dx of the other
rows are what they are without them.

What it does not do, loudly: ``Tiled`` grids, ``Nearest`` / ``Smoothstep`` interpolation, inputs other than 3-D,
``n_features_per_level`` outside {1, 2, 4, 8}, more than 32 levels, half precision, CPU tensors.  The initial parameters are
uniform in [-1e-4, 1e-4] from a torch generator seeded with ``seed`` (tiny-cuda-nn's range; its PRNG stream is not reproduced).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _capi
from .tet_spheres_ext import _device_ctx, _stream_ptr

__all__ = ["GridEncoding", "GridPointPlan", "parse_grid_config", "grid_layout", "sorted_workspace_bytes", "plan_bytes",
           "planned_workspace_bytes"]

_lib = _capi.load()

_OTYPES = {"hashgrid": "Hash", "densegrid": "Dense", "grid": None}


PARAM_GRAD_MODES = ("atomic", "sorted")


def parse_grid_config(n_input_dims: int, config: dict, param_grad: str | None = None) -> dict:
    """The accepted ``tcnn.Encoding`` grid configs, normalised; ValueError on anything else.  ``param_grad`` (the keyword, else
    the config key of that name, else ``"atomic"``) picks the route to dL/dparams: ``"atomic"`` (float atomics, last bits may
    differ between runs) or ``"sorted"`` (radix sort + fixed-order sums, bitwise repeatable; csrc/grid.h states the contract)."""
    cfg = dict(config)
    otype = str(cfg.get("otype", "")).lower()
    if otype not in _OTYPES:
        raise ValueError(f"tssplat_amd encoding: otype {cfg.get('otype')!r} is not offered (HashGrid, DenseGrid, Grid only)")
    gtype = _OTYPES[otype] or str(cfg.get("type", "Hash"))
    if gtype not in ("Hash", "Dense"):
        raise ValueError(f"tssplat_amd encoding: grid type {gtype!r} is not offered (Hash or Dense; Tiled is not)")
    if n_input_dims != 3:
        raise ValueError(f"tssplat_amd encoding: n_input_dims = {n_input_dims}: only 3-D inputs are offered")
    interp = cfg.get("interpolation", "Linear")
    if interp != "Linear":
        raise ValueError(f"tssplat_amd encoding: interpolation {interp!r} is not offered (Linear only)")
    out = {
        "n_levels": int(cfg.get("n_levels", 16)),
        "n_features_per_level": int(cfg.get("n_features_per_level", 2)),
        "log2_hashmap_size": int(cfg.get("log2_hashmap_size", 19)),
        "base_resolution": int(cfg.get("base_resolution", 16)),
        "per_level_scale": float(cfg.get("per_level_scale", 2.0)),
        "dense": gtype == "Dense",
        "param_grad": cfg.get("param_grad", "atomic") if param_grad is None else param_grad,
    }
    if out["param_grad"] not in PARAM_GRAD_MODES:
        raise ValueError(f"tssplat_amd encoding: param_grad = {out['param_grad']!r} ('atomic' or 'sorted' only)")
    if out["n_features_per_level"] not in (1, 2, 4, 8):
        raise ValueError(f"tssplat_amd encoding: n_features_per_level = {out['n_features_per_level']} (1, 2, 4 or 8 only)")
    return out


def _args(cfg: dict) -> tuple:
    return (cfg["n_levels"], cfg["n_features_per_level"], cfg["log2_hashmap_size"], cfg["base_resolution"],
            C.c_float(cfg["per_level_scale"]), int(cfg["dense"]))


def grid_layout(cfg: dict) -> dict:
    """Per-level first entry (``offset``, L + 1 values), ``res``, ``is_hash``, float32 ``scale`` and ``n_params`` (tsamd_grid_layout)."""
    L = cfg["n_levels"]
    off = np.zeros(L + 1, np.int64)
    res = np.zeros(L, np.int32)
    hashed = np.zeros(L, np.int32)
    scale = np.zeros(L, np.float32)
    n = C.c_int64(0)
    _capi.check(_lib.tsamd_grid_layout(*_args(cfg), off.ctypes.data, res.ctypes.data, hashed.ctypes.data, scale.ctypes.data, C.byref(n)))
    return {"offset": off, "res": res, "is_hash": hashed.astype(bool), "scale": scale, "n_params": int(n.value)}


def grid_layout_n_params(cfg: dict) -> int:
    n = C.c_int64(0)
    _capi.check(_lib.tsamd_grid_layout(*_args(cfg), None, None, None, None, C.byref(n)))
    return int(n.value)


def _bytes_query(query, cfg: dict, n_points: int) -> int:
    n = C.c_int64(0)
    _capi.check(query(int(n_points), *_args(cfg), C.byref(n)))
    return int(n.value)


def sorted_workspace_bytes(cfg: dict, n_points: int) -> int:
    """Bytes of workspace the sorted backward needs for ``n_points`` (tsamd_grid_backward_sorted_workspace_bytes; host only)."""
    return _bytes_query(_lib.tsamd_grid_backward_sorted_workspace_bytes, cfg, n_points)


def plan_bytes(cfg: dict, n_points: int) -> int:
    """Bytes of a point plan for ``n_points`` (tsamd_grid_plan_bytes; host only)."""
    return _bytes_query(_lib.tsamd_grid_plan_bytes, cfg, n_points)


def planned_workspace_bytes(cfg: dict, n_points: int) -> int:
    """Bytes of workspace the planned backward needs (tsamd_grid_backward_planned_workspace_bytes; host only)."""
    return _bytes_query(_lib.tsamd_grid_backward_planned_workspace_bytes, cfg, n_points)


PLAN_KEYS = ("n_levels", "n_features_per_level", "log2_hashmap_size", "base_resolution", "per_level_scale", "dense")


class GridPointPlan:
    """A frozen point set, sorted once for the planned dL/dparams (csrc/grid.h states the contract).  ``x``: the plan's own
    contiguous copy of the points (no gradient: a planned point set is frozen); ``cfg``: the normalised config it was built
    for; ``buffer``: the device plan; ``nbytes``: its size.  Build one with :meth:`GridEncoding.plan_points`."""

    def __init__(self, x: torch.Tensor, cfg: dict):
        self.x = x.detach().clone(memory_format=torch.contiguous_format)
        self.x.requires_grad_(False)
        self.n_points = int(self.x.shape[0])
        self.cfg = {k: cfg[k] for k in PLAN_KEYS}
        dev = self.x.device
        self.buffer = torch.empty(plan_bytes(cfg, self.n_points), dtype=torch.uint8, device=dev)
        with _device_ctx(dev):
            ws = torch.empty(sorted_workspace_bytes(cfg, self.n_points), dtype=torch.uint8, device=dev)
            _capi.check(_lib.tsamd_grid_plan_build(self.x.data_ptr(), self.n_points, *_args(cfg), self.buffer.data_ptr(), self.buffer.numel(),
                                                   ws.data_ptr(), ws.numel(), _stream_ptr(dev)))

    @property
    def nbytes(self) -> int:
        return int(self.buffer.numel())

    @property
    def device(self) -> torch.device:
        return self.x.device

    def check_cfg(self, cfg: dict) -> None:
        """ValueError unless ``cfg`` (normalised) is the config this plan was built for."""
        mine, theirs = self.cfg, {k: cfg[k] for k in PLAN_KEYS}
        if mine != theirs:
            raise ValueError(f"tssplat_amd encoding: this point plan was built for {mine}, not for {theirs}")


def _check_input(x: torch.Tensor, n_input_dims: int) -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError("tssplat_amd encoding: x must be a GPU tensor (there is no CPU fallback)")
    if x.dtype != torch.float32:
        raise RuntimeError("tssplat_amd encoding: x must be float32")
    if x.dim() != 2 or x.shape[1] != n_input_dims:
        raise RuntimeError(f"tssplat_amd encoding: x must be [N, {n_input_dims}], got {tuple(x.shape)}")
    return x.contiguous()


def _encode(x: torch.Tensor, params: torch.Tensor, cfg: dict, n_output_dims: int) -> torch.Tensor:
    N = int(x.shape[0])
    out = torch.empty((N, n_output_dims), dtype=torch.float32, device=x.device)
    with _device_ctx(x.device):
        _capi.check(_lib.tsamd_grid_encode(x.data_ptr(), N, params.data_ptr(), *_args(cfg), out.data_ptr(), _stream_ptr(x.device)))
    return out


class _GridEncodeFunc(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, params, cfg, n_output_dims):
        ctx.cfg = cfg
        ctx.save_for_backward(x, params)
        return _encode(x, params, cfg, n_output_dims)

    @staticmethod
    def backward(ctx, grad_out):
        x, params = ctx.saved_tensors
        need_x, need_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_x or need_p):
            return None, None, None, None
        g = grad_out.contiguous()
        N = int(x.shape[0])
        grad_p = torch.zeros_like(params) if need_p else None
        grad_x = torch.empty_like(x) if need_x else None
        ptr = lambda t: None if t is None else t.data_ptr()
        with _device_ctx(x.device):
            if ctx.cfg["param_grad"] == "sorted" and need_p:
                ws = torch.empty(sorted_workspace_bytes(ctx.cfg, N), dtype=torch.uint8, device=x.device)
                _capi.check(_lib.tsamd_grid_encode_backward_sorted(x.data_ptr(), N, params.data_ptr(), *_args(ctx.cfg), g.data_ptr(),
                                                                   ptr(grad_p), ptr(grad_x), ws.data_ptr(), ws.numel(),
                                                                   _stream_ptr(x.device)))
            else:
                _capi.check(_lib.tsamd_grid_encode_backward(x.data_ptr(), N, params.data_ptr(), *_args(ctx.cfg), g.data_ptr(),
                                                            ptr(grad_p), ptr(grad_x), _stream_ptr(x.device)))
        return grad_x, grad_p, None, None


class _GridEncodePlannedFunc(torch.autograd.Function):
    """The encode forward on ``plan.x`` (the same kernel: the same bits); dL/dparams by the planned route, whatever param_grad."""

    @staticmethod
    def forward(ctx, params, plan, cfg, n_output_dims):
        ctx.cfg, ctx.plan = cfg, plan
        return _encode(plan.x, params, cfg, n_output_dims)

    @staticmethod
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        plan, cfg = ctx.plan, ctx.cfg
        g = grad_out.contiguous()
        dev = plan.x.device
        grad_p = torch.zeros(grid_layout_n_params(cfg), dtype=torch.float32, device=dev)
        with _device_ctx(dev):
            ws = torch.empty(planned_workspace_bytes(cfg, plan.n_points), dtype=torch.uint8, device=dev)
            _capi.check(_lib.tsamd_grid_encode_backward_planned(plan.x.data_ptr(), plan.n_points, *_args(cfg), g.data_ptr(), grad_p.data_ptr(),
                                                                plan.buffer.data_ptr(), plan.buffer.numel(), ws.data_ptr(), ws.numel(),
                                                                _stream_ptr(dev)))
        return grad_p, None, None, None


def encode_planned(plan: GridPointPlan, params: torch.Tensor, cfg: dict, n_output_dims: int) -> torch.Tensor:
    """``encode(plan.x)`` with the planned backward; ValueError on a plan built for another config."""
    if not isinstance(plan, GridPointPlan):
        raise TypeError("tssplat_amd encoding: expected a GridPointPlan")
    plan.check_cfg(cfg)
    if not params.is_cuda or params.device != plan.x.device:
        raise RuntimeError("tssplat_amd encoding: params and the plan's points must live on the same GPU")
    return _GridEncodePlannedFunc.apply(params, plan, cfg, n_output_dims)


class GridEncoding(torch.nn.Module):
    """``tcnn.Encoding(3, grid_config)``: ``forward(x [N, 3] fp32 on the GPU) -> [N, n_levels * n_features_per_level]``."""

    def __init__(self, n_input_dims: int, config: dict, seed: int = 1337, param_grad: str | None = None):
        super().__init__()
        self.cfg = parse_grid_config(n_input_dims, config, param_grad)
        self.layout = grid_layout(self.cfg)
        self.n_input_dims = n_input_dims
        self.n_output_dims = self.cfg["n_levels"] * self.cfg["n_features_per_level"]
        gen = torch.Generator().manual_seed(int(seed))
        init = torch.rand(self.layout["n_params"], generator=gen, dtype=torch.float32) * 2e-4 - 1e-4
        dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.params = torch.nn.Parameter(init.to(dev))

    def plan_points(self, x: torch.Tensor) -> GridPointPlan:
        """Sorts a frozen point set once (``x``: as for ``forward``).  ``forward(plan)`` then gives ``forward(plan.x)``'s bits,
        and its dL/dparams is the sorted route's, bit for bit, without the sort: no float atomics, a few launches.  The plan
        owns a copy of ``x``; it carries no gradient to any ``x``.  It costs ``8 * n_levels * 4`` bytes per point."""
        return GridPointPlan(_check_input(x, self.n_input_dims), self.cfg)

    def forward(self, x) -> torch.Tensor:
        if isinstance(x, GridPointPlan):
            return encode_planned(x, self.params, self.cfg, self.n_output_dims)
        x = _check_input(x, self.n_input_dims)
        if not self.params.is_cuda or self.params.device != x.device:
            raise RuntimeError("tssplat_amd encoding: params and x must live on the same GPU")
        return _GridEncodeFunc.apply(x, self.params, self.cfg, self.n_output_dims)

    def extra_repr(self) -> str:
        c = self.cfg
        return (f"{'Dense' if c['dense'] else 'Hash'}, n_levels={c['n_levels']}, F={c['n_features_per_level']}, "
                f"log2_T={c['log2_hashmap_size']}, base={c['base_resolution']}, per_level_scale={c['per_level_scale']:.6g}, "
                f"n_params={self.layout['n_params']}, param_grad={c['param_grad']}")

