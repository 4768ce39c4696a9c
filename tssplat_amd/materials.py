"""Mirror of the reference's ``materials/`` (/root/reference/materials/explicit_material.py, materials/__init__.py): the texture
stage's colour field, a hash-grid encoding (:mod:`tssplat_amd.encoding`) feeding a small MLP, queried by
``MeshRasterizer`` at every foreground pixel (renderers/mesh_rasterizer.py:111-128; :class:`tssplat_amd.renderers.MeshRasterizer`
takes it unchanged as ``materials``).

Same ``Config`` defaults, ``contract_to_unisphere``, forward and ``export`` (``material.pth``) as the reference; the config is a
dict (the reference's ``parse_structured`` builds an OmegaConf node from the same dataclass).
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import Any, Dict, Optional

import torch

from .encoding import GridPointPlan
from .models import get_activation, get_encoding, get_mlp, scale_tensor, _rank

__all__ = ["ExplicitMaterial", "contract_to_unisphere", "load_material"]


def contract_to_unisphere(x, bbox, unbounded: bool = False):
    """explicit_material.py:17-29."""
    if unbounded:
        x = scale_tensor(x, bbox, (0, 1))
        x = x * 2 - 1
        mag = x.norm(dim=-1, keepdim=True)
        mask = mag.squeeze(-1) > 1
        x[mask] = (2 - 1 / mag[mask]) * (x[mask] / mag[mask])
        x = x / 4 + 0.5
    else:
        x = scale_tensor(x, bbox, (0, 1))
    return x


class ExplicitMaterial(torch.nn.Module):
    """explicit_material.py:32-112."""

    @dataclass
    class Config:
        n_output_dims: int
        material_activation: str
        pos_encoding_config: dict = field(default_factory=lambda: {
            "otype": "HashGrid",
            "n_levels": 16,
            "n_features_per_level": 2,
            "log2_hashmap_size": 19,
            "base_resolution": 16,
            "per_level_scale": 1.447269237440378,
        })
        mlp_network_config: dict = field(default_factory=lambda: {
            "otype": "VanillaMLP",
            "activation": "ReLU",
            "output_activation": "none",
            "n_neurons": 64,
            "n_hidden_layers": 1,
        })

    def __init__(self, cfg: Optional[dict] = None):
        super().__init__()
        self.cfg = self.Config(**dict(cfg or {}))
        self.device = torch.device(f"cuda:{_rank()}")
        self.register_buffer("bbox", torch.as_tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]], dtype=torch.float32))
        self.encoding = get_encoding(3, self.cfg.pos_encoding_config)
        self.feature_network = get_mlp(self.encoding.n_output_dims, self.cfg.n_output_dims, self.cfg.mlp_network_config)
        self.to(self.device)

    def plan_points(self, positions) -> GridPointPlan:
        """A point plan for a frozen set of surface points: ``positions`` contracted exactly as ``forward`` does, flattened to
        ``[-1, 3]`` and planned through the grid encoding.  ``forward(positions=plan)`` then returns the colour of those
        points, ``[n_points, 3]``, with the planned (sort-free, atomic-free) dL/dparams of the grid."""
        with torch.no_grad():
            x = contract_to_unisphere(positions, self.bbox)
            return self.encoding.plan_points(x.reshape(-1, 3))

    def forward(self, positions, **kwargs) -> Dict[str, Any]:
        if isinstance(positions, GridPointPlan):
            features = self.feature_network(self.encoding(positions)).view(positions.n_points, 3)
            return {"color": get_activation(self.cfg.material_activation)(features)}
        positions = contract_to_unisphere(positions, self.bbox)          # points normalised to (0, 1)
        enc = self.encoding(positions.view(-1, 3))
        features = self.feature_network(enc).view(*positions.shape[:-1], 3)
        color = get_activation(self.cfg.material_activation)(features)
        return {"color": color}

    def export(self, path: str, folder: str):
        os.makedirs(os.path.join(path, folder), exist_ok=True)
        torch.save(self.state_dict(), os.path.join(path, folder, "material.pth"))


def load_material(material_class_type):
    """materials/__init__.py:4-9."""
    if material_class_type == "ExplicitMaterial":
        return ExplicitMaterial
    raise NotImplementedError(f"Unknown geometry class type: {material_class_type}")
