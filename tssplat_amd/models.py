"""Mirror of the reference's ``models/networks.py`` over :mod:`tssplat_amd.tcnn`: the encodings and MLPs the texture stage's
``ExplicitMaterial`` builds (/root/reference/materials/explicit_material.py:62-69).

Same names, same constructor arguments and the same forward arithmetic as the reference; configs are plain dicts (or any
object with ``.get`` / attribute access, such as an OmegaConf node) instead of the reference's OmegaConf plumbing
(``config_to_primitive``, networks.py:52-53).  ``tcnn.Encoding`` is the HIP grid encoding; the tcnn network routes
(``TCNNNetwork``, ``TCNNNetworkWithInputEncoding``) run the HIP fused MLP for otypes FullyFusedMLP / CutlassMLP / MLP and raise
for other otypes, as :mod:`tssplat_amd.tcnn` does.
"""
from __future__ import annotations

import math
from typing import Callable

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import tcnn
from .encoding import GridPointPlan

__all__ = ["get_activation", "get_encoding", "get_mlp", "scale_tensor", "TCNNEncoding", "ProgressiveBandHashGrid",
           "ProgressiveBandFrequency", "CompositeEncoding", "VanillaMLP", "SphereInitVanillaMLP", "TCNNNetwork",
           "NetworkWithInputEncoding", "TCNNNetworkWithInputEncoding", "create_network_with_input_encoding", "ToDTypeWrapper"]


def _get(config, key, default=None):
    if isinstance(config, dict):
        return config.get(key, default)
    return config.get(key, default) if hasattr(config, "get") else getattr(config, key, default)


def _primitive(config) -> dict:
    if isinstance(config, dict):
        return dict(config)
    try:                                                        # an OmegaConf node
        from omegaconf import OmegaConf
        return OmegaConf.to_container(config, resolve=True)
    except ImportError:
        return dict(config)


def _rank() -> int:
    """utils/config.py:get_rank (networks.py:11)."""
    import os
    for key in ("RANK", "LOCAL_RANK", "SLURM_PROCID", "JSM_NAMESPACE_RANK"):
        if os.environ.get(key) is not None:
            return int(os.environ[key])
    return 0


def get_activation(name) -> Callable:
    """networks.py:16-49."""
    if name is None:
        return lambda x: x
    name = name.lower()
    if name == "none":
        return lambda x: x
    if name == "lin2srgb":
        return lambda x: torch.where(x > 0.0031308, torch.pow(torch.clamp(x, min=0.0031308), 1.0 / 2.4) * 1.055 - 0.055,
                                     12.92 * x).clamp(0.0, 1.0)
    if name == "exp":
        return lambda x: torch.exp(x)
    if name == "shifted_exp":
        return lambda x: torch.exp(x - 1.0)
    if name == "sigmoid":
        return lambda x: torch.sigmoid(x)
    if name == "tanh":
        return lambda x: torch.tanh(x)
    if name == "shifted_softplus":
        return lambda x: F.softplus(x - 1.0)
    if name == "scale_-11_01":
        return lambda x: x * 0.5 + 0.5
    try:
        return getattr(F, name)
    except AttributeError:
        raise ValueError(f"Unknown activation function: {name}")


class ProgressiveBandFrequency(nn.Module):
    """networks.py:56-94."""

    def __init__(self, in_channels: int, config: dict):
        super().__init__()
        self.N_freqs = config["n_frequencies"]
        self.in_channels, self.n_input_dims = in_channels, in_channels
        self.funcs = [torch.sin, torch.cos]
        self.freq_bands = 2 ** torch.linspace(0, self.N_freqs - 1, self.N_freqs)
        self.n_output_dims = self.in_channels * (len(self.funcs) * self.N_freqs)
        self.n_masking_step = config.get("n_masking_step", 0)
        self.update_step(None, None)

    def forward(self, x):
        out = []
        for freq, mask in zip(self.freq_bands, self.mask):
            for func in self.funcs:
                out += [func(freq * x) * mask]
        return torch.cat(out, -1)

    def update_step(self, epoch, global_step, on_load_weights=False):
        if self.n_masking_step <= 0 or global_step is None:
            self.mask = torch.ones(self.N_freqs, dtype=torch.float32)
        else:
            self.mask = (1.0 - torch.cos(math.pi * (global_step / self.n_masking_step * self.N_freqs
                                                    - torch.arange(0, self.N_freqs)).clamp(0, 1))) / 2.0


class TCNNEncoding(nn.Module):
    """networks.py:97-106."""

    def __init__(self, in_channels, config, dtype=torch.float32) -> None:
        super().__init__()
        self.n_input_dims = in_channels
        with torch.cuda.device(_rank()):
            self.encoding = tcnn.Encoding(in_channels, config, dtype=dtype)
        self.n_output_dims = self.encoding.n_output_dims

    def forward(self, x):
        return self.encoding(x)

    def plan_points(self, x):
        """A point plan of the grid encoding (:meth:`tssplat_amd.encoding.GridEncoding.plan_points`); ``forward`` takes it."""
        return self.encoding.plan_points(x)


class ProgressiveBandHashGrid(nn.Module):
    """networks.py:109-148."""

    def __init__(self, in_channels, config, dtype=torch.float32):
        super().__init__()
        self.n_input_dims = in_channels
        encoding_config = config.copy()
        encoding_config["otype"] = "Grid"
        encoding_config["type"] = "Hash"
        with torch.cuda.device(_rank()):
            self.encoding = tcnn.Encoding(in_channels, encoding_config, dtype=dtype)
        self.n_output_dims = self.encoding.n_output_dims
        self.n_level = config["n_levels"]
        self.n_features_per_level = config["n_features_per_level"]
        self.start_level, self.start_step, self.update_steps = config["start_level"], config["start_step"], config["update_steps"]
        self.current_level = self.start_level
        self.mask = torch.zeros(self.n_level * self.n_features_per_level, dtype=torch.float32, device=_rank())

    def forward(self, x):
        return self.encoding(x) * self.mask

    def plan_points(self, x):
        """A point plan of the grid encoding (:meth:`tssplat_amd.encoding.GridEncoding.plan_points`); ``forward`` takes it."""
        return self.encoding.plan_points(x)

    def update_step(self, epoch, global_step, on_load_weights=False):
        current_level = min(self.start_level + max(global_step - self.start_step, 0) // self.update_steps, self.n_level)
        self.current_level = current_level
        self.mask[: self.current_level * self.n_features_per_level] = 1.0


class CompositeEncoding(nn.Module):
    """networks.py:151-172."""

    def __init__(self, encoding, include_xyz=False, xyz_scale=2.0, xyz_offset=-1.0):
        super().__init__()
        self.encoding = encoding
        self.include_xyz, self.xyz_scale, self.xyz_offset = include_xyz, xyz_scale, xyz_offset
        self.n_output_dims = int(self.include_xyz) * self.encoding.n_input_dims + self.encoding.n_output_dims

    def forward(self, x, *args):
        if not self.include_xyz:
            return self.encoding(x, *args)
        xyz = x.x if isinstance(x, GridPointPlan) else x            # (a plan's xyz columns come from its own points)
        return torch.cat([xyz * self.xyz_scale + self.xyz_offset, self.encoding(x, *args)], dim=-1)

    def plan_points(self, x):
        """A point plan of the wrapped grid encoding; ``forward(plan)`` takes it in place of ``x``."""
        if not hasattr(self.encoding, "plan_points"):
            raise NotImplementedError(f"{type(self.encoding).__name__} offers no point plan (grid encodings only)")
        return self.encoding.plan_points(x)


def get_encoding(n_input_dims: int, config) -> nn.Module:
    """networks.py:175-192 (input in [0, 1])."""
    otype = _get(config, "otype")
    if otype == "ProgressiveBandFrequency":
        encoding = ProgressiveBandFrequency(n_input_dims, _primitive(config))
    elif otype == "ProgressiveBandHashGrid":
        encoding = ProgressiveBandHashGrid(n_input_dims, _primitive(config))
    else:
        encoding = TCNNEncoding(n_input_dims, _primitive(config))
    return CompositeEncoding(encoding, include_xyz=_get(config, "include_xyz", False), xyz_scale=2.0, xyz_offset=-1.0)


class VanillaMLP(nn.Module):
    """networks.py:195-235: bias-free Linear layers, ReLU, an output activation."""

    def __init__(self, dim_in: int, dim_out: int, config: dict):
        super().__init__()
        self.n_neurons, self.n_hidden_layers = config["n_neurons"], config["n_hidden_layers"]
        layers = [self.make_linear(dim_in, self.n_neurons, is_first=True, is_last=False), self.make_activation()]
        for _ in range(self.n_hidden_layers - 1):
            layers += [self.make_linear(self.n_neurons, self.n_neurons, is_first=False, is_last=False), self.make_activation()]
        layers += [self.make_linear(self.n_neurons, dim_out, is_first=False, is_last=True)]
        self.layers = nn.Sequential(*layers)
        self.output_activation = get_activation(config.get("output_activation", None))

    def forward(self, x):
        with torch.autocast("cuda", enabled=False):
            return self.output_activation(self.layers(x))

    def make_linear(self, dim_in, dim_out, is_first, is_last):
        return nn.Linear(dim_in, dim_out, bias=False)

    def make_activation(self):
        return nn.ReLU(inplace=True)


class SphereInitVanillaMLP(nn.Module):
    """networks.py:238-311: geometric initialisation, weight norm, Softplus(beta=100)."""

    def __init__(self, dim_in, dim_out, config):
        super().__init__()
        self.n_neurons, self.n_hidden_layers = config["n_neurons"], config["n_hidden_layers"]
        self.sphere_init, self.weight_norm = True, True
        self.sphere_init_radius = config["sphere_init_radius"]
        self.sphere_init_inside_out = config["inside_out"]
        layers = [self.make_linear(dim_in, self.n_neurons, is_first=True, is_last=False), self.make_activation()]
        for _ in range(self.n_hidden_layers - 1):
            layers += [self.make_linear(self.n_neurons, self.n_neurons, is_first=False, is_last=False), self.make_activation()]
        layers += [self.make_linear(self.n_neurons, dim_out, is_first=False, is_last=True)]
        self.layers = nn.Sequential(*layers)
        self.output_activation = get_activation(config.get("output_activation", None))

    def forward(self, x):
        with torch.autocast("cuda", enabled=False):
            return self.output_activation(self.layers(x))

    def make_linear(self, dim_in, dim_out, is_first, is_last):
        layer = nn.Linear(dim_in, dim_out, bias=True)
        if is_last:
            sign = -1.0 if self.sphere_init_inside_out else 1.0
            torch.nn.init.constant_(layer.bias, -sign * self.sphere_init_radius)
            torch.nn.init.normal_(layer.weight, mean=sign * math.sqrt(math.pi) / math.sqrt(dim_in), std=0.0001)
        elif is_first:
            torch.nn.init.constant_(layer.bias, 0.0)
            torch.nn.init.constant_(layer.weight[:, 3:], 0.0)
            torch.nn.init.normal_(layer.weight[:, :3], 0.0, math.sqrt(2) / math.sqrt(dim_out))
        else:
            torch.nn.init.constant_(layer.bias, 0.0)
            torch.nn.init.normal_(layer.weight, 0.0, math.sqrt(2) / math.sqrt(dim_out))
        if self.weight_norm:
            layer = nn.utils.weight_norm(layer)
        return layer

    def make_activation(self):
        return nn.Softplus(beta=100)


class TCNNNetwork(nn.Module):
    """networks.py:314-321: ``tcnn.Network`` (the HIP fused MLP), output cast to float32."""

    def __init__(self, dim_in: int, dim_out: int, config: dict) -> None:
        super().__init__()
        with torch.cuda.device(_rank()):
            self.network = tcnn.Network(dim_in, dim_out, config)

    def forward(self, x):
        return self.network(x).float()


def get_mlp(n_input_dims, n_output_dims, config) -> nn.Module:
    """networks.py:324-339; the tcnn route is ``TCNNNetwork`` (the HIP fused MLP; otypes other than FullyFusedMLP /
    CutlassMLP / MLP raise through tssplat_amd.tcnn.Network)."""
    otype = _get(config, "otype")
    if otype == "VanillaMLP":
        return VanillaMLP(n_input_dims, n_output_dims, _primitive(config))
    if otype == "SphereInitVanillaMLP":
        return SphereInitVanillaMLP(n_input_dims, n_output_dims, _primitive(config))
    assert _get(config, "sphere_init", False) is False, "sphere_init=True only supported by VanillaMLP"
    return TCNNNetwork(n_input_dims, n_output_dims, _primitive(config))


class NetworkWithInputEncoding(nn.Module):
    """networks.py:342-348."""

    def __init__(self, encoding, network):
        super().__init__()
        self.encoding, self.network = encoding, network

    def forward(self, x):
        return self.network(self.encoding(x))


class TCNNNetworkWithInputEncoding(nn.Module):
    """networks.py:351-371: ``tcnn.NetworkWithInputEncoding`` (grid encoding + HIP fused MLP), output cast to float32."""

    def __init__(self, n_input_dims: int, n_output_dims: int, encoding_config: dict, network_config: dict) -> None:
        super().__init__()
        with torch.cuda.device(_rank()):
            self.network_with_input_encoding = tcnn.NetworkWithInputEncoding(
                n_input_dims=n_input_dims, n_output_dims=n_output_dims, encoding_config=encoding_config,
                network_config=network_config)

    def forward(self, x):
        return self.network_with_input_encoding(x).float()


def create_network_with_input_encoding(n_input_dims: int, n_output_dims: int, encoding_config, network_config) -> nn.Module:
    """networks.py:374-394 (input in [0, 1])."""
    if _get(encoding_config, "otype") in ["VanillaFrequency", "ProgressiveBandHashGrid"] or \
            _get(network_config, "otype") in ["VanillaMLP", "SphereInitVanillaMLP"]:
        encoding = get_encoding(n_input_dims, encoding_config)
        network = get_mlp(encoding.n_output_dims, n_output_dims, network_config)
        return NetworkWithInputEncoding(encoding, network)
    return TCNNNetworkWithInputEncoding(n_input_dims=n_input_dims, n_output_dims=n_output_dims,
                                        encoding_config=_primitive(encoding_config), network_config=_primitive(network_config))


class ToDTypeWrapper(nn.Module):
    """networks.py:397-404."""

    def __init__(self, module: nn.Module, dtype: torch.dtype):
        super().__init__()
        self.module = module
        self.dtype = dtype

    def forward(self, x):
        return self.module(x).to(self.dtype)


def scale_tensor(dat, inp_scale, tgt_scale):
    """networks.py:407-419."""
    if inp_scale is None:
        inp_scale = (0, 1)
    if tgt_scale is None:
        tgt_scale = (0, 1)
    if isinstance(tgt_scale, torch.Tensor):
        assert dat.shape[-1] == tgt_scale.shape[-1]
    dat = (dat - inp_scale[0]) / (inp_scale[1] - inp_scale[0])
    return dat * (tgt_scale[1] - tgt_scale[0]) + tgt_scale[0]
