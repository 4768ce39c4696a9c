"""Voxelising triangle meshes on the device: the integer winding number on the merge's grid, occupancy and volume IoU.

``merge.occupancy`` knows the inside of a union of tets; this module knows the inside of a triangle mesh, by the signed crossing
count along grid columns -- the winding number of Jacobson et al. discretised with Pineda's edge functions and fill rule.  Vertices
snap to a lattice of ``2^-10`` node spacings, coverage of a column by a face is an exact int64 predicate with a tie rule that gives a
shared edge to exactly one of its two faces, and a covered column receives ``-sign(area)`` at the first node behind the crossing; the
inclusive prefix sum along the ray is ``w``: +1 inside a closed surface whose normals point outwards, additive over faces, negated
when every face is reversed.  Overlapping closed components add up (``"nonzero"`` is their union), interior sheets cancel, and a
defect spoils only the columns it touches: ``open_columns`` counts those, and ``rays=3`` out-votes them with the other two axes.
The kernels sit behind ``tsamd_voxel_winding`` and ``tsamd_voxel_occupancy`` (include/tssplat_amd.h); the sums are integers, so the
result is bitwise repeatable, and tests/voxel_oracle.py is the same statement in numpy and the definition.  There is no CPU fallback.

Grid: the merge's -- ``G`` nodes per axis (1 .. 512) over ``[lo, hi]^3``, node ``(i, j, k)`` at ``lo + (index + 0.5) h``.

Limits.  A crossing that ties with a node, and the lattice snap (``h 2^-11`` at most), are decided per axis, so the three rays may
disagree at nodes the surface passes through (``disputed``).  A face whose box of candidate columns is large is walked by one wave;
a mesh of many such faces is slow by construction.

Out of scope: an exact float winding number, sparse workspaces, 16-bit deposits.
"""
from __future__ import annotations

import dataclasses
import functools

import torch

from . import _args, _capi, merge

__all__ = ["VoxelWinding", "VoxelOccupancy", "winding", "occupancy", "mesh_volume_iou", "workspace_bytes", "RULES", "MIN_GRID", "MAX_GRID", "SUBCELL_BITS",
           "LANE_COLUMNS"]

MIN_GRID = 1
MAX_GRID = 512
SUBCELL_BITS = 10
LANE_COLUMNS = 16         # csrc/voxel.h: a face with more candidate columns is walked by its whole wave
RULES = {"nonzero": _capi.TSAMD_VOXEL_NONZERO, "positive": _capi.TSAMD_VOXEL_POSITIVE, "odd": _capi.TSAMD_VOXEL_ODD}     # include/tssplat_amd.h
_STATS = 12
_COUNT_WORDS = 64 * _STATS * 2       # csrc/voxel.h: 64 copies of the counts, in int32 words, ahead of the deposits


@dataclasses.dataclass
class VoxelWinding:
    """``w``: int32 ``[G, G, G]`` in the (i, j, k) layout whatever the axis.  ``open_columns``: columns of the ray whose deposits do not sum
    to 0 (none on a closed mesh).  ``invalid_faces``: faces with an index out of range or a corner that is not finite or farther than
    ``2^19`` nodes from ``lo``; ``degenerate_faces``: valid faces whose projection along the ray has no area; ``deposits``: covered
    (face, column) pairs; ``wave_faces``: faces with more than ``LANE_COLUMNS`` candidate columns, which a whole wave walked."""
    w: torch.Tensor
    open_columns: int
    invalid_faces: int
    degenerate_faces: int
    deposits: int
    wave_faces: int = 0


@dataclasses.dataclass
class VoxelOccupancy:
    """``occ``: bool ``[G, G, G]``.  ``open_columns``, ``degenerate_faces`` and ``deposits``: one entry per ray (three, or one for ``rays=1``).
    ``disputed``: nodes at which the three rays' bits differ (0 for ``rays=1``).  ``wave_faces`` sums over the rays."""
    occ: torch.Tensor
    open_columns: tuple
    disputed: int
    invalid_faces: int
    degenerate_faces: tuple
    deposits: tuple = ()
    wave_faces: int = 0


# ---- argument checks: the shared ones live in tssplat_amd/_args.py; here are the order and what only this module checks ----
_fail = functools.partial(_args.fail, "voxelize")
_ptr = _args.ptr


def _check_mesh(name: str, v, faces, v_arg: str = "v", f_arg: str = "faces", device=None):
    """Types and shapes of both first, then where they live; a tensor that is not contiguous is copied."""
    v, faces = _args.triangle_mesh(_fail, name, v, faces, 2 ** 31 - 1, v_arg, f_arg, device)
    return v.contiguous(), faces.contiguous()


def _check_rays(name: str, rays) -> int:
    if not _args.is_int(rays) or int(rays) not in (1, 3):
        _fail(name, f"rays must be 1 or 3, got {rays!r}")
    return int(rays)


def workspace_bytes(grid: int) -> int:
    """``tsamd_voxel_workspace_bytes``: room for the counts' copies and three rays' deposits, ``6144 + 3 (G + 1) G^2 x 4`` bytes."""
    return int(_capi.load().tsamd_voxel_workspace_bytes(_args.integer(_fail, "workspace_bytes", "grid", grid, MIN_GRID, MAX_GRID)))


def _winding(v, faces, grid, lo, hi, axis):
    """(w, stats): enqueued; ``stats`` is the int64 record on the device."""
    dev = v.device
    lib, ctx, stream = _args.lib_and_stream(dev)
    ws = torch.empty(_COUNT_WORDS + (grid + 1) * grid * grid, dtype=torch.int32, device=dev)
    w = torch.empty((grid, grid, grid), dtype=torch.int32, device=dev)
    stats = torch.empty(_STATS, dtype=torch.int64, device=dev)
    with ctx:
        _capi.check(lib.tsamd_voxel_winding(_ptr(v), int(v.shape[0]), _ptr(faces), int(faces.shape[0]), grid, lo, hi, axis, ws.data_ptr(), w.data_ptr(),
                                            stats.data_ptr(), stream))
    return w, stats


def _occupancy(v, faces, grid, lo, hi, rule, rays):
    """(occ, stats): enqueued."""
    dev = v.device
    lib, ctx, stream = _args.lib_and_stream(dev)
    ws = torch.empty(_COUNT_WORDS + rays * (grid + 1) * grid * grid, dtype=torch.int32, device=dev)
    occ = torch.empty((grid, grid, grid), dtype=torch.uint8, device=dev)
    stats = torch.empty(_STATS, dtype=torch.int64, device=dev)
    with ctx:
        _capi.check(lib.tsamd_voxel_occupancy(_ptr(v), int(v.shape[0]), _ptr(faces), int(faces.shape[0]), grid, lo, hi, RULES[rule], rays, ws.data_ptr(),
                                              occ.data_ptr(), stats.data_ptr(), stream))
    return occ.view(torch.bool), stats                                   # the kernels write 0 or 1


def _occupancy_record(occ, s, rays) -> VoxelOccupancy:
    s = [int(x) for x in s]
    return VoxelOccupancy(occ, tuple(s[0:rays]), s[3], s[4], tuple(s[5:5 + rays]), tuple(s[8:8 + rays]), s[11])


def winding(v: torch.Tensor, faces: torch.Tensor, grid: int, bounds, axis: int = 0) -> VoxelWinding:
    """The winding number of the mesh ``v`` float32 ``[Nv, 3]``, ``faces`` int32 ``[Nt, 3]`` at the ``grid``^3 nodes over ``bounds = (lo, hi)``,
    counted along ``axis`` (0: rays along i, 1: j, 2: k).  Parts of the mesh outside the cube are clipped; what lies before the first
    node of a column still counts for it.  One readback: the counts."""
    name = "winding"
    grid = _args.integer(_fail, name, "grid", grid, MIN_GRID, MAX_GRID)
    lo, hi = _args.bounds(_fail, name, bounds, grid)
    if not _args.is_int(axis, 0, 2):
        _fail(name, f"axis must be 0, 1 or 2, got {axis!r}")
    axis = int(axis)
    v, faces = _check_mesh(name, v, faces)
    w, stats = _winding(v, faces, grid, lo, hi, axis)
    s = [int(x) for x in stats.cpu().numpy()]
    return VoxelWinding(w, s[axis], s[4], s[5 + axis], s[8 + axis], s[11])


def occupancy(v: torch.Tensor, faces: torch.Tensor, grid: int, bounds, rule: str = "nonzero", rays: int = 3) -> VoxelOccupancy:
    """The inside nodes of the mesh: ``rule`` applied to the winding number -- ``"nonzero"`` (the union of overlapping closed parts),
    ``"positive"`` or ``"odd"``.  ``rays=1`` counts along axis 0; ``rays=3`` takes the majority of the three axes' bits, which out-votes a
    column spoilt by a hole or a fin of the mesh.  No winding array is written.  One readback: the counts."""
    name = "occupancy"
    grid = _args.integer(_fail, name, "grid", grid, MIN_GRID, MAX_GRID)
    lo, hi = _args.bounds(_fail, name, bounds, grid)
    rule = _args.choice(_fail, name, "rule", rule, RULES)
    rays = _check_rays(name, rays)
    v, faces = _check_mesh(name, v, faces)
    occ, stats = _occupancy(v, faces, grid, lo, hi, rule, rays)
    return _occupancy_record(occ, stats.cpu().numpy(), rays)


def mesh_volume_iou(v_a: torch.Tensor, f_a: torch.Tensor, v_b: torch.Tensor, f_b: torch.Tensor, grid: int = 128, bounds=None, rule: str = "nonzero", rays: int = 3) -> dict:
    """Intersection over union of the two meshes' occupancies on one grid: ``dict(iou, inside_a, inside_b, a, b, grid, bounds)`` with ``iou``
    as :func:`tssplat_amd.merge.volume_iou` states it (two integer counts; 1.0 when both are empty) and ``a`` / ``b`` the
    :class:`VoxelOccupancy` records.  ``bounds=None``: :func:`tssplat_amd.merge.default_bounds` over both vertex sets (``grid >= 5``; one
    more readback).  One readback: both records and the four counts."""
    name = "mesh_volume_iou"
    grid = _args.integer(_fail, name, "grid", grid, MIN_GRID, MAX_GRID)
    rule = _args.choice(_fail, name, "rule", rule, RULES)
    rays = _check_rays(name, rays)
    if bounds is not None:
        bounds = _args.bounds(_fail, name, bounds, grid)
    v_a, f_a = _check_mesh(name, v_a, f_a, "v_a", "f_a")
    v_b, f_b = _check_mesh(name, v_b, f_b, "v_b", "f_b", v_a.device)
    lo, hi = _args.bounds(_fail, name, merge.default_bounds(torch.cat([v_a, v_b]), grid), grid) if bounds is None else bounds
    occ_a, stats_a = _occupancy(v_a, f_a, grid, lo, hi, rule, rays)
    occ_b, stats_b = _occupancy(v_b, f_b, grid, lo, hi, rule, rays)
    counts = torch.stack([(occ_a & occ_b).sum(), (occ_a | occ_b).sum(), occ_a.sum(), occ_b.sum()])
    host = torch.cat([counts, stats_a, stats_b]).cpu().numpy()
    inter, union, inside_a, inside_b = (int(x) for x in host[:4])
    return {"iou": merge.iou_of_counts(inter, union), "inside_a": inside_a, "inside_b": inside_b,
            "a": _occupancy_record(occ_a, host[4:4 + _STATS], rays), "b": _occupancy_record(occ_b, host[4 + _STATS:], rays), "grid": grid, "bounds": (lo, hi)}
