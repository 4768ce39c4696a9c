"""A ``tinycudann``-named stand-in: ``import tssplat_amd.tcnn as tcnn`` where the reference does ``import tinycudann as tcnn``
(models/networks.py:2).  tiny-cuda-nn is a CUDA-only library; what the reference's texture stage takes from it is the grid
encoding (``tcnn.Encoding``, models/networks.py:97-106 and :113-116), served here by the HIP kernels of
:mod:`tssplat_amd.encoding`, and the fully fused MLP (``tcnn.Network``, ``tcnn.NetworkWithInputEncoding``,
models/networks.py:314-404) for network otypes ``FullyFusedMLP`` / ``CutlassMLP`` / ``MLP``, served by the HIP kernels of
:mod:`tssplat_amd.network`.  Other network otypes raise ``NotImplementedError``: the reference's default MLP is
``VanillaMLP`` (plain ``nn.Linear``, models/networks.py:195-235), which needs nothing from here.
"""
from __future__ import annotations

import torch

from .encoding import GridEncoding, GridPointPlan, _GridEncodeFunc, _check_input, encode_planned
from .network import FusedMLP, fused_mlp, is_network_otype

__all__ = ["Encoding", "Network", "NetworkWithInputEncoding"]


class Encoding(GridEncoding):
    """``tcnn.Encoding(n_input_dims, encoding_config, seed=1337, dtype=None)`` for the grid encodings (HashGrid, DenseGrid,
    Grid with type Hash / Dense); fp32 only.  ``param_grad`` ("atomic" | "sorted", also a config key) is this package's own:
    the route to dL/dparams (:func:`tssplat_amd.encoding.parse_grid_config`)."""

    def __init__(self, n_input_dims: int, encoding_config: dict, seed: int = 1337, dtype=None, param_grad: str | None = None):
        if dtype not in (None, torch.float32):
            raise ValueError(f"tssplat_amd.tcnn.Encoding: dtype {dtype} is not offered (float32 only)")
        super().__init__(n_input_dims, encoding_config, seed=seed, param_grad=param_grad)


def _check_network_otype(cls: str, network_config) -> None:
    otype = network_config.get("otype") if network_config is not None else None
    if not is_network_otype(otype):
        raise NotImplementedError(f"tssplat_amd.tcnn.{cls}: network otype {otype!r} is not offered (FullyFusedMLP, CutlassMLP or "
                                  "MLP); use the VanillaMLP route (mlp_network_config otype 'VanillaMLP', plain nn.Linear)")


class Network(FusedMLP):
    """``tcnn.Network(n_input_dims, n_output_dims, network_config, seed=1337)``: the fused MLP of :mod:`tssplat_amd.network`;
    float32 output."""

    def __init__(self, n_input_dims: int, n_output_dims: int, network_config: dict, seed: int = 1337):
        _check_network_otype("Network", network_config)
        super().__init__(n_input_dims, n_output_dims, network_config, seed=seed)


class NetworkWithInputEncoding(torch.nn.Module):
    """``tcnn.NetworkWithInputEncoding(n_input_dims, n_output_dims, encoding_config, network_config, seed=1337)``: the grid
    encoding followed by the fused MLP.  ``params`` is one Parameter, ``[network params | encoding params]`` (tiny-cuda-nn's
    order, unpinned), split in two by views."""

    def __init__(self, n_input_dims: int, n_output_dims: int, encoding_config: dict, network_config: dict = None, seed: int = 1337,
                 param_grad: str | None = None):
        super().__init__()
        _check_network_otype("NetworkWithInputEncoding", network_config)     # before the encoding config is parsed
        enc = GridEncoding(n_input_dims, encoding_config, seed=seed, param_grad=param_grad)
        net = FusedMLP(enc.n_output_dims, n_output_dims, network_config, seed=seed)
        self.encoding_cfg, self.network_cfg = enc.cfg, net.cfg
        self.n_input_dims, self.n_output_dims = int(n_input_dims), int(n_output_dims)
        self.n_network_params = net.layout["n_params"]
        self.params = torch.nn.Parameter(torch.cat([net.params.detach(), enc.params.detach()]))

    @property
    def network_params(self) -> torch.Tensor:
        return self.params[: self.n_network_params]

    @property
    def encoding_params(self) -> torch.Tensor:
        return self.params[self.n_network_params:]

    def plan_points(self, x: torch.Tensor) -> GridPointPlan:
        """:meth:`tssplat_amd.encoding.GridEncoding.plan_points` for this module's encoding; ``forward(plan)`` takes it."""
        return GridPointPlan(_check_input(x, self.n_input_dims), self.encoding_cfg)

    def forward(self, x) -> torch.Tensor:
        if isinstance(x, GridPointPlan):
            features = encode_planned(x, self.encoding_params, self.encoding_cfg, self.network_cfg["n_input_dims"])
            return fused_mlp(features, self.network_params, self.network_cfg)
        x = _check_input(x, self.n_input_dims)
        if not self.params.is_cuda or self.params.device != x.device:
            raise RuntimeError("tssplat_amd network: params and x must live on the same GPU")
        features = _GridEncodeFunc.apply(x, self.encoding_params, self.encoding_cfg, self.network_cfg["n_input_dims"])
        return fused_mlp(features, self.network_params, self.network_cfg)
