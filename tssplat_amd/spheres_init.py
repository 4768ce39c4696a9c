"""Sphere initialisation on the device: silhouettes -> visual hull -> exact squared distance transform -> greedy ball cover.

The first stage of the pipeline: the job of the reference's data/generate_init_spheres.py, which writes the key-point file
``{"pt": [...], "r": [...]}`` that ``TetMeshMultiSphereGeometry`` starts from (geometry/tetmesh_geometry.py:233-243).  The
reference selects its spheres from a skeleton by a MILP; that is NOT rebuilt here ("Sphere initialisation").  This is
the project's own placement -- the largest inscribed ball of the still-uncovered part of the visual hull, repeated -- as HIP
kernels behind ``tsamd_hull_carve``, ``tsamd_edt_squared`` and ``tsamd_greedy_cover`` (include/tssplat_amd.h), stated in integers
so that it is bitwise repeatable; tests/spheres_init_oracle.py is the same statement in numpy.  There is no CPU fallback.

Grid: ``G = grid`` voxels per axis (1 .. 512) over the cube ``[lo, hi]^3``, ``h = (hi - lo) / G``; voxel ``(i, j, k)`` has the C-order
flat index ``(i G + j) G + k`` and the centre ``lo + (index + 0.5) h`` per axis.
"""
from __future__ import annotations

import dataclasses
import functools
import json
import math
from typing import Optional

import numpy as np
import torch

from . import _args, _capi

__all__ = ["KeyPoints", "visual_hull", "distance_transform_sq", "greedy_cover", "init_spheres", "cover_occupancy", "voxel_centres", "MAX_GRID"]

MAX_GRID = 512           # 3 x 511^2 < 2^31: squared distances are int32
_MAX_SPHERES = 1 << 20   # include/tssplat_amd.h: tsamd_greedy_cover


@dataclasses.dataclass
class KeyPoints:
    """Sphere centres and radii: the content of the reference's key-point file.  ``hull_fraction`` (hull voxels over all voxels) and
    ``uncovered_fraction`` (hull voxels no ball covers over hull voxels) describe the placement that made them; a file does not
    carry them (``None`` after ``load_json``)."""
    pt: np.ndarray                                  # float32 [S, 3]
    r: np.ndarray                                   # float32 [S]
    hull_fraction: Optional[float] = None
    uncovered_fraction: Optional[float] = None

    def __post_init__(self):
        self.pt = np.ascontiguousarray(np.asarray(self.pt, dtype=np.float32).reshape(-1, 3))
        self.r = np.ascontiguousarray(np.asarray(self.r, dtype=np.float32).reshape(-1))
        if self.pt.shape[0] != self.r.shape[0]:
            raise ValueError(f"KeyPoints: {self.pt.shape[0]} centres but {self.r.shape[0]} radii")

    def __len__(self) -> int:
        return int(self.r.shape[0])

    def save_json(self, path) -> None:
        """The layout generate_init_spheres.py:536-543 writes: ``"pt"`` a list of ``[x, y, z]``, ``"r"`` a list of one-element lists."""
        with open(path, "w") as fh:
            json.dump({"pt": self.pt.astype(np.float64).tolist(), "r": self.r.astype(np.float64).reshape(-1, 1).tolist()}, fh, indent=4)

    @classmethod
    def load_json(cls, path) -> "KeyPoints":
        """Reads what ``save_json`` and the reference's script write (``"r"`` as one-element lists or as plain numbers)."""
        with open(path, "r") as fh:
            skel = json.load(fh)
        return cls(np.asarray(skel["pt"], dtype=np.float64).reshape(-1, 3), np.asarray(skel["r"], dtype=np.float64).reshape(-1))


# ---- argument checks: the shared ones live in tssplat_amd/_args.py; here are the order and what only this module checks ----
_fail = functools.partial(_args.fail, "spheres_init")


def _tensor(name: str, arg: str, t, dtype, device=None) -> torch.Tensor:
    """On a GPU, of ``dtype``, on ``device``; a tensor that is not contiguous is copied."""
    return _args.gpu_tensor(_fail, name, arg, t, dtype, device).contiguous()


def _check_volume(name: str, arg: str, t, dtype, device=None, grid=None) -> torch.Tensor:
    t = _tensor(name, arg, t, dtype, device)
    if t.dim() != 3 or not (t.shape[0] == t.shape[1] == t.shape[2]) or not 1 <= t.shape[0] <= MAX_GRID or (grid is not None and t.shape[0] != grid):
        want = f"[{grid}, {grid}, {grid}]" if grid is not None else f"[G, G, G] with G in 1 .. {MAX_GRID}"
        _fail(name, f"{arg} must be {want}, got {tuple(t.shape)}")
    return t


def _check_cover_params(name: str, n_spheres, min_radius, shrink):
    n_spheres = _args.integer(_fail, name, "n_spheres", n_spheres, 0, _MAX_SPHERES, "2^20")
    min_radius, shrink = float(min_radius), float(shrink)
    if not (math.isfinite(min_radius) and min_radius >= 0.0):
        _fail(name, f"min_radius must be finite and not negative, got {min_radius!r}")
    if not (math.isfinite(shrink) and shrink > 0.0):
        _fail(name, f"shrink must be finite and positive, got {shrink!r}")
    return n_spheres, min_radius, shrink


def voxel_centres(grid: int, bounds=(-1.0, 1.0)) -> np.ndarray:
    """float32 ``[G]``: the voxel centres along one axis, ``lo + (index + 0.5) h`` in float64, rounded once."""
    grid = _args.integer(_fail, "voxel_centres", "grid", grid, 1, MAX_GRID)
    lo, hi = _args.bounds(_fail, "voxel_centres", bounds)
    h = (hi - lo) / grid
    return (lo + (np.arange(grid, dtype=np.float64) + 0.5) * h).astype(np.float32)


def _cover_constants(grid: int, lo: float, hi: float, min_radius: float, shrink: float):
    h = (hi - lo) / grid
    return h, shrink * shrink, (h * shrink) * (h * shrink), min_radius * min_radius


# ---- the three stages ----
def _hull(name, alpha, mvp, grid, bounds, threshold, channel) -> torch.Tensor:
    grid = _args.integer(_fail, name, "grid", grid, 1, MAX_GRID)
    lo, hi = _args.bounds(_fail, name, bounds)
    alpha = _tensor(name, "alpha", alpha, torch.float32)
    if alpha.dim() != 4 or alpha.shape[0] < 1 or alpha.shape[3] < 1 or not (1 <= alpha.shape[1] <= 8192 and 1 <= alpha.shape[2] <= 8192):
        _fail(name, f"alpha must be [B, H, W, C] with B, C >= 1 and H, W in 1 .. 8192, got {tuple(alpha.shape)}")
    B, H, W, Cn = (int(s) for s in alpha.shape)
    mvp = _tensor(name, "mvp", mvp, torch.float32, alpha.device)
    if tuple(mvp.shape) != (B, 4, 4):
        _fail(name, f"mvp must be [{B}, 4, 4] (one matrix per view of alpha), got {tuple(mvp.shape)}")
    channel = _args.integer(_fail, name, "channel", channel, 0, Cn - 1)
    threshold = float(threshold)
    if math.isnan(threshold):
        _fail(name, "threshold is NaN")
    lib, ctx, stream = _args.lib_and_stream(alpha.device)
    bits = torch.empty((B, H, (W + 31) // 32), dtype=torch.int32, device=alpha.device)
    hull = torch.empty((grid, grid, grid), dtype=torch.bool, device=alpha.device)
    with ctx:
        _capi.check(lib.tsamd_hull_carve(alpha.data_ptr(), B, H, W, Cn, channel, threshold, mvp.data_ptr(), grid, lo, hi, bits.data_ptr(),
                                         hull.data_ptr(), stream))
    return hull


def visual_hull(alpha: torch.Tensor, mvp: torch.Tensor, grid: int = 72, bounds=(-1.0, 1.0), threshold: float = 0.5, channel: int = 0) -> torch.Tensor:
    """bool ``[G, G, G]``: the voxels whose centre every view sees on the object.

    ``alpha`` float32 ``[B, H, W, C]`` (row 0 at ``ndc_y = -1``, as ``dr.rasterize`` writes), ``mvp`` float32 ``[B, 4, 4]``.  A voxel
    centre ``p`` is inside view ``b`` iff ``clip = mvp[b] (p, 1)`` (float32, every multiply and add rounded on its own) has
    ``clip_w > 0``, ``|clip_x / clip_w| < 1``, ``|clip_y / clip_w| < 1`` and ``alpha[b, py, px, channel] > threshold`` at the pixel the
    point falls into.  A NaN anywhere makes the comparison false: outside."""
    return _hull("visual_hull", alpha, mvp, grid, bounds, threshold, channel)


def _edt(mask: torch.Tensor):
    """(d2, status): enqueues the three passes; ``status`` (one int32 on the device) is 1 when the mask has a false voxel."""
    G = int(mask.shape[0])
    lib, ctx, stream = _args.lib_and_stream(mask.device)
    d2 = torch.empty((G, G, G), dtype=torch.int32, device=mask.device)
    ws = torch.empty((G, G, G), dtype=torch.int32, device=mask.device)
    status = torch.empty(1, dtype=torch.int32, device=mask.device)
    with ctx:
        _capi.check(lib.tsamd_edt_squared(mask.data_ptr(), G, ws.data_ptr(), d2.data_ptr(), status.data_ptr(), stream))
    return d2, status


def distance_transform_sq(mask: torch.Tensor) -> torch.Tensor:
    """int32 ``[G, G, G]``: the exact squared distance, in voxel units, from every voxel to the nearest voxel whose mask is false
    (0 where it is false).  Nothing outside the array counts as background: ``scipy.ndimage.distance_transform_edt(mask) ** 2``.
    A mask without a false voxel has no transform: ``ValueError`` (found on the device; the passes after the first do nothing then)."""
    mask = _check_volume("distance_transform_sq", "mask", mask, torch.bool)
    d2, status = _edt(mask)
    if int(status.item()) == 0:
        raise ValueError("tssplat_amd.spheres_init.distance_transform_sq: mask has no false voxel")
    return d2


def _cover(hull, d2, n_spheres, lo, hi, min_radius, shrink):
    """(flat, q, count, uncovered) on the device: ``count`` launches record a ball, nothing synchronises."""
    G = int(hull.shape[0])
    _, s2, hs2, m2 = _cover_constants(G, lo, hi, min_radius, shrink)
    lib, ctx, stream = _args.lib_and_stream(hull.device)
    dev = hull.device
    ws = torch.empty(n_spheres + 1, dtype=torch.int64, device=dev)
    uncovered = torch.empty_like(hull)
    flat = torch.empty(n_spheres, dtype=torch.int32, device=dev)
    q = torch.empty(n_spheres, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    with ctx:
        _capi.check(lib.tsamd_greedy_cover(hull.data_ptr(), d2.data_ptr(), G, n_spheres, s2, hs2, m2, ws.data_ptr(), uncovered.data_ptr(), _args.ptr(flat),
                                           _args.ptr(q), count.data_ptr(), stream))
    return flat, q, count, uncovered


def greedy_cover(hull: torch.Tensor, d2: torch.Tensor, n_spheres: int, bounds=(-1.0, 1.0), min_radius: float = 0.05, shrink: float = 0.92):
    """``(flat int64 [S], q int32 [S], uncovered bool [G, G, G])``.  At most ``n_spheres`` times: take ``q = max d2`` over the uncovered
    voxels (at first the hull), the lowest flat index among equals; stop when nothing is uncovered, ``q == 0`` or the radius
    ``sqrt(q) h shrink`` is below ``min_radius`` (tested as ``q (h shrink)^2 < min_radius^2`` in float64); record ``(flat, q)`` and
    clear every voxel within ``sqrt(q) shrink`` voxels of it (``D2 <= q shrink^2``, one float64 product)."""
    hull = _check_volume("greedy_cover", "hull", hull, torch.bool)
    d2 = _check_volume("greedy_cover", "d2", d2, torch.int32, hull.device, int(hull.shape[0]))
    lo, hi = _args.bounds(_fail, "greedy_cover", bounds)
    n_spheres, min_radius, shrink = _check_cover_params("greedy_cover", n_spheres, min_radius, shrink)
    flat, q, count, uncovered = _cover(hull, d2, n_spheres, lo, hi, min_radius, shrink)
    S = int(count.item())                                    # the one readback
    return flat[:S].long(), q[:S].clone(), uncovered


def init_spheres(alpha: torch.Tensor, mvp: torch.Tensor, n_spheres: int, grid: int = 72, bounds=(-1.0, 1.0), threshold: float = 0.5, channel: int = 0,
                 min_radius: float = 0.05, shrink: float = 0.92) -> KeyPoints:
    """Key points for ``TetMeshMultiSphereGeometry`` from silhouettes: ``visual_hull``, ``distance_transform_sq`` and ``greedy_cover``
    enqueued back to back, one readback at the end.  Centres are voxel centres (float32), radii ``float32(sqrt(q) h shrink)``.
    A hull that fills the whole cube has no distance transform: ``ValueError``."""
    name = "init_spheres"
    n_spheres, min_radius, shrink = _check_cover_params(name, n_spheres, min_radius, shrink)
    hull = _hull(name, alpha, mvp, grid, bounds, threshold, channel)
    lo, hi = _args.bounds(_fail, name, bounds)
    return _cover_occupancy(name, hull, n_spheres, lo, hi, min_radius, shrink, "the visual hull")


def _cover_occupancy(name, occ, n_spheres, lo, hi, min_radius, shrink, what) -> KeyPoints:
    """The distance transform and the cover of a checked occupancy grid, enqueued back to back, and the one readback."""
    G = int(occ.shape[0])
    d2, status = _edt(occ)
    flat, q, count, uncovered = _cover(occ, d2, n_spheres, lo, hi, min_radius, shrink)
    # one packed readback: status, count, hull voxels, uncovered voxels, then the records
    head = torch.stack([status[0].long(), count[0].long(), occ.sum(), uncovered.sum()])
    host = torch.cat([head, flat.long(), q.long()]).cpu().numpy()
    if int(host[0]) == 0:
        raise ValueError(f"tssplat_amd.spheres_init.{name}: {what} fills the whole grid (no false voxel): nothing bounds the object")
    S, n_hull, n_left = int(host[1]), int(host[2]), int(host[3])
    flat_h, q_h = host[4:4 + S], host[4 + n_spheres:4 + n_spheres + S]
    c = voxel_centres(G, (lo, hi))
    h = (hi - lo) / G
    ijk = np.stack(np.unravel_index(flat_h, (G, G, G)), axis=1).reshape(-1, 3)
    r = (np.sqrt(q_h.astype(np.float64)) * h * shrink).astype(np.float32)
    return KeyPoints(c[ijk].reshape(-1, 3), r, hull_fraction=n_hull / float(G ** 3), uncovered_fraction=n_left / float(max(1, n_hull)))


def cover_occupancy(occ: torch.Tensor, n_spheres: int, bounds=(-1.0, 1.0), min_radius: float = 0.05, shrink: float = 0.92) -> KeyPoints:
    """Key points from any occupancy grid ``occ`` bool ``[G, G, G]`` over ``bounds`` -- a visual hull, or the voxelised target mesh
    (:func:`tssplat_amd.voxelize.occupancy`): the tail of :func:`init_spheres`, ``distance_transform_sq`` and ``greedy_cover`` enqueued back
    to back with one readback.  ``hull_fraction`` is the occupied fraction of the grid.  A grid without a false voxel: ``ValueError``."""
    name = "cover_occupancy"
    occ = _check_volume(name, "occ", occ, torch.bool)
    lo, hi = _args.bounds(_fail, name, bounds)
    n_spheres, min_radius, shrink = _check_cover_params(name, n_spheres, min_radius, shrink)
    return _cover_occupancy(name, occ, n_spheres, lo, hi, min_radius, shrink, "occ")
