"""Fully fused MLP on the gfx950 kernels (csrc/mlp_kernels.hip): tiny-cuda-nn's ``FullyFusedMLP`` / ``CutlassMLP`` behind
``tcnn.Network`` and ``tcnn.NetworkWithInputEncoding`` (models/networks.py:314-321 and :342-404).

Semantics: tests/mlp_oracle.py -- PARITY UNPINNED against the library itself (CUDA only, not available here).  Bias-free;
fp16 operands, fp32 sums; ``params`` is one flat float32 vector of L + 1 row-major [out, in] matrices ([W, in_w],
(L - 1) x [W, W], [out_w, W], the widths padded to multiples of 16, padded input columns reading 1.0).  The output is
float32 (tiny-cuda-nn returns half; every caller in the reference applies ``.float()``), so the incoming gradient is not
rounded to half before the loss scale 128 is applied.  ``S * dy`` above 65504 is not guarded, as in the library.

What it does not do, loudly: widths other than 16 / 32 / 64 / 128, more than 8 hidden layers, more than 256 inputs or 64
outputs, hidden activations other than ReLU / None, output activations other than None / Sigmoid, fp16 parameters, CPU
tensors.  The initial matrices are xavier-uniform over their padded shapes from a torch generator seeded with ``seed``
(tiny-cuda-nn's PRNG stream is not reproduced).
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _capi
from .tet_spheres_ext import _device_ctx, _stream_ptr

__all__ = ["FusedMLP", "parse_mlp_config", "mlp_layout", "ACTIVATIONS", "OUTPUT_ACTIVATIONS"]

_lib = _capi.load()

NETWORK_OTYPES = ("fullyfusedmlp", "cutlassmlp", "mlp")
ACTIVATIONS = {"relu": _capi.TSAMD_MLP_ACT_RELU, "none": _capi.TSAMD_MLP_ACT_NONE}                  # include/tssplat_amd.h
OUTPUT_ACTIVATIONS = {"none": 0, "sigmoid": 2}
WIDTHS = (16, 32, 64, 128)
LOSS_SCALE = 128.0


def is_network_otype(otype) -> bool:
    return isinstance(otype, str) and otype.lower() in NETWORK_OTYPES


def parse_mlp_config(n_input_dims: int, n_output_dims: int, config: dict) -> dict:
    """The accepted ``tcnn.Network`` configs, normalised; ValueError on a value outside the envelope.  The caller has
    already checked that ``otype`` names a fused network (see :func:`is_network_otype`)."""
    cfg = dict(config)
    width = int(cfg.get("n_neurons", 128))
    hidden = int(cfg.get("n_hidden_layers", 5))
    act = str(cfg.get("activation", "ReLU"))
    out_act = str(cfg.get("output_activation", "None"))
    if width not in WIDTHS:
        raise ValueError(f"tssplat_amd network: n_neurons = {width} is not offered (16, 32, 64 or 128)")
    if not 1 <= hidden <= 8:
        raise ValueError(f"tssplat_amd network: n_hidden_layers = {hidden} is not offered (1 .. 8)")
    if act.lower() not in ACTIVATIONS:
        raise ValueError(f"tssplat_amd network: activation {act!r} is not offered (ReLU or None)")
    if out_act.lower() not in OUTPUT_ACTIVATIONS:
        raise ValueError(f"tssplat_amd network: output_activation {out_act!r} is not offered (None or Sigmoid)")
    if not 1 <= int(n_input_dims) <= 256:
        raise ValueError(f"tssplat_amd network: n_input_dims = {n_input_dims} is not offered (1 .. 256)")
    if not 1 <= int(n_output_dims) <= 64:
        raise ValueError(f"tssplat_amd network: n_output_dims = {n_output_dims} is not offered (1 .. 64)")
    return {"n_input_dims": int(n_input_dims), "n_output_dims": int(n_output_dims), "n_neurons": width, "n_hidden_layers": hidden,
            "activation": ACTIVATIONS[act.lower()], "output_activation": OUTPUT_ACTIVATIONS[out_act.lower()]}


def _args(cfg: dict) -> tuple:
    return (cfg["n_input_dims"], cfg["n_output_dims"], cfg["n_neurons"], cfg["n_hidden_layers"], cfg["activation"],
            cfg["output_activation"])


def mlp_layout(cfg: dict) -> dict:
    """``n_params``, ``in_w``, ``out_w`` and the matrix shapes (tsamd_mlp_layout for the counts)."""
    n = C.c_int64(0)
    in_w, out_w = C.c_int32(0), C.c_int32(0)
    _capi.check(_lib.tsamd_mlp_layout(*_args(cfg), C.byref(n), C.byref(in_w), C.byref(out_w)))
    W, L = cfg["n_neurons"], cfg["n_hidden_layers"]
    shapes = [(W, in_w.value)] + [(W, W)] * (L - 1) + [(out_w.value, W)]
    return {"n_params": int(n.value), "in_w": int(in_w.value), "out_w": int(out_w.value), "shapes": shapes}


def xavier_init(layout: dict, seed: int) -> torch.Tensor:
    """Each matrix uniform in +-sqrt(6 / (rows + cols)) over its padded shape, from a CPU generator seeded with ``seed``."""
    gen = torch.Generator().manual_seed(int(seed))
    parts = []
    for rows, cols in layout["shapes"]:
        bound = math.sqrt(6.0 / (rows + cols))
        parts.append((torch.rand(rows * cols, generator=gen, dtype=torch.float32) * 2.0 - 1.0) * bound)
    return torch.cat(parts)


def _check_input(x: torch.Tensor, n_input_dims: int) -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError("tssplat_amd network: x must be a GPU tensor (there is no CPU fallback)")
    if x.dim() != 2 or x.shape[1] != n_input_dims:
        raise RuntimeError(f"tssplat_amd network: x must be [N, {n_input_dims}], got {tuple(x.shape)}")
    return x.float().contiguous()                      # tiny-cuda-nn's binding casts the input as well


class _FusedMLPFunc(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, params, cfg):
        N = int(x.shape[0])
        y = torch.empty((N, cfg["n_output_dims"]), dtype=torch.float32, device=x.device)
        if N > 0:
            with _device_ctx(x.device):
                _capi.check(_lib.tsamd_mlp_forward(x.data_ptr(), N, params.data_ptr(), *_args(cfg), y.data_ptr(), _stream_ptr(x.device)))
        ctx.cfg = cfg
        ctx.save_for_backward(x, params)
        return y

    @staticmethod
    def backward(ctx, grad_y):
        x, params = ctx.saved_tensors
        need_x, need_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_x or need_p):
            return None, None, None
        N = int(x.shape[0])
        if N == 0:
            return (torch.zeros_like(x) if need_x else None), (torch.zeros_like(params) if need_p else None), None
        g = grad_y.float().contiguous()
        grad_p = torch.empty_like(params) if need_p else None
        grad_x = torch.empty_like(x) if need_x else None
        ws = None
        if need_p:
            nbytes = int(_lib.tsamd_mlp_workspace_bytes(N, *_args(ctx.cfg)))
            if nbytes < 0:
                _capi.check(1)
            ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)
        with _device_ctx(x.device):
            _capi.check(_lib.tsamd_mlp_backward(x.data_ptr(), N, params.data_ptr(), *_args(ctx.cfg), g.data_ptr(),
                                                None if grad_p is None else grad_p.data_ptr(),
                                                None if grad_x is None else grad_x.data_ptr(),
                                                None if ws is None else ws.data_ptr(), _stream_ptr(x.device)))
        return grad_x, grad_p, None


def fused_mlp(x: torch.Tensor, params: torch.Tensor, cfg: dict) -> torch.Tensor:
    """The fused MLP as a function of ``x`` [N, n_input_dims] and the flat ``params`` (both on one GPU)."""
    x = _check_input(x, cfg["n_input_dims"])
    if not params.is_cuda or params.device != x.device or params.dtype != torch.float32:
        raise RuntimeError("tssplat_amd network: params must be float32 on the GPU of x")
    return _FusedMLPFunc.apply(x, params, cfg)


class FusedMLP(torch.nn.Module):
    """``tcnn.Network(n_input_dims, n_output_dims, config)``: ``forward(x [N, n_input_dims]) -> [N, n_output_dims]`` float32."""

    def __init__(self, n_input_dims: int, n_output_dims: int, config: dict, seed: int = 1337):
        super().__init__()
        self.cfg = parse_mlp_config(n_input_dims, n_output_dims, config)
        self.layout = mlp_layout(self.cfg)
        self.n_input_dims, self.n_output_dims = int(n_input_dims), int(n_output_dims)
        init = xavier_init(self.layout, seed)
        dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.params = torch.nn.Parameter(init.to(dev))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return fused_mlp(x, self.params, self.cfg)

    def extra_repr(self) -> str:
        c = self.cfg
        return (f"{c['n_input_dims']} -> {c['n_neurons']} x {c['n_hidden_layers']} -> {c['n_output_dims']}, "
                f"activation={c['activation']}, output_activation={c['output_activation']}, n_params={self.layout['n_params']}")
