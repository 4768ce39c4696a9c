"""A ``tinycudann``-named stand-in: ``import tssplat_amd.tcnn as tcnn`` where the reference does ``import tinycudann as tcnn``
(models/networks.py:2).  tiny-cuda-nn is a CUDA-only library; what the reference's texture stage takes from it is the grid
encoding (``tcnn.Encoding``, models/networks.py:97-106 and :113-116), served here by the HIP kernels of
:mod:`tssplat_amd.encoding`.  The fused MLPs (``tcnn.Network``, ``tcnn.NetworkWithInputEncoding``) are not offered: the
reference's default MLP is ``VanillaMLP`` (plain ``nn.Linear``, models/networks.py:195-235), which needs nothing from here.
"""
from __future__ import annotations

import torch

from .encoding import GridEncoding

__all__ = ["Encoding", "Network", "NetworkWithInputEncoding"]


class Encoding(GridEncoding):
    """``tcnn.Encoding(n_input_dims, encoding_config, seed=1337, dtype=None)`` for the grid encodings (HashGrid, DenseGrid,
    Grid with type Hash / Dense); fp32 only."""

    def __init__(self, n_input_dims: int, encoding_config: dict, seed: int = 1337, dtype=None):
        if dtype not in (None, torch.float32):
            raise ValueError(f"tssplat_amd.tcnn.Encoding: dtype {dtype} is not offered (float32 only)")
        super().__init__(n_input_dims, encoding_config, seed=seed)


class Network(torch.nn.Module):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("tssplat_amd.tcnn.Network: tiny-cuda-nn's fused MLPs are not offered; use the "
                                  "VanillaMLP route (mlp_network_config otype 'VanillaMLP', plain nn.Linear)")


class NetworkWithInputEncoding(torch.nn.Module):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("tssplat_amd.tcnn.NetworkWithInputEncoding: tiny-cuda-nn's fused MLPs are not offered; use "
                                  "tcnn.Encoding followed by the VanillaMLP route (plain nn.Linear)")
