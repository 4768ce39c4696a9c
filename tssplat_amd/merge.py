"""Merging the fitted tet-spheres into one closed surface on the device: tet mesh -> union field -> marching tetrahedra.

The reference's README hands this step to TetWild ("merge the optimized TetSpheres into one shape").  TetWild is NOT rebuilt
here, and parity with its output is not a goal.  This is the project's own merge, in the style of the sphere initialisation: HIP
kernels behind ``tsamd_union_field``, ``tsamd_surface_count`` and ``tsamd_surface_emit`` (include/tssplat_amd.h), stated in
separately rounded float64 operations and integer maxima so that it is bitwise repeatable; tests/union_oracle.py is the same
statement in numpy.  There is no CPU fallback.

Flood fill (``tsamd_grid_components``, ``tsamd_field_fill``; tests/fill_oracle.py): the extraction gives one closed surface per
boundary between an inside and an outside component of the grid's nodes, under the connectivity of the extraction itself (a node
and node +- (di, dj, dk), (di, dj, dk) in {0, 1}^3 without 0: 14 neighbours).  :func:`components` labels both kinds of component
with their smallest flat index; :func:`fill_field` makes enclosed outside components inside (``"cavities"``) and then keeps only
the largest solid component (``"outer"``); ``merge_tets(fill=...)`` extracts the filled field, whose surface is a sub-mesh of the
unfilled one: the same vertex bits in the same order, without the removed components.

Grid: the one of :mod:`tssplat_amd.spheres_init` -- ``G = grid`` nodes per axis (2 .. 512) over the cube ``[lo, hi]^3``,
``h = (hi - lo) / G``, node ``(i, j, k)`` at ``lo + (index + 0.5) h`` per axis (float64), flat index ``(i G + j) G + k``.

Simplification: ``merge_tets(simplify=k)`` clusters the extracted surface on ``grid // k`` cells per axis of the same cube
(:mod:`tssplat_amd.simplify`: vertex clustering with quadric placement; it does not preserve manifoldness, so ``closed`` is then
what :func:`tssplat_amd.simplify.edge_stats` finds).

Smoothing: ``merge_tets(smooth=n)`` runs ``n`` iterations of the default mode of :mod:`tssplat_amd.smooth` (Taubin's filter) on the
surface that is handed out, after the fill and the simplification.  It moves vertices only: ``faces``, and with them ``closed``, stay.

Out of scope: re-tetrahedralising.
"""
from __future__ import annotations

import dataclasses
import functools
import math
from typing import Optional

import numpy as np
import torch

from . import _args, _capi

__all__ = ["MergedSurface", "FilledField", "union_field", "extract_surface", "merge_tets", "components", "fill_field", "occupancy", "volume_iou", "iou_of_counts",
           "default_bounds", "default_level", "write_obj", "MIN_GRID", "MAX_GRID", "FILL_MODES"]

MIN_GRID = 2
MAX_GRID = 512           # flat node indices < 2^27; 7 vertices and 12 triangles per node stay below 2^31
_MAX_TETS = 1 << 30      # include/tssplat_amd.h: tsamd_union_field
FILL_MODES = {"cavities": _capi.TSAMD_FILL_CAVITIES, "outer": _capi.TSAMD_FILL_OUTER}      # include/tssplat_amd.h


@dataclasses.dataclass
class MergedSurface:
    """One indexed triangle mesh around the union of all tets.  ``closed``: no grid-border node is inside, so every edge lies in
    exactly two triangles of opposite direction.  ``inside_fraction``: inside nodes over all nodes, of the field that was extracted.
    ``fill``: ``"none"``, ``"cavities"`` or ``"outer"``, and what it changed (:class:`FilledField`).  ``simplified``: set by ``merge_tets(simplify=k)``;
    ``v`` / ``faces`` then are the clustered mesh and ``closed`` is what ``simplify.edge_stats`` finds on it.  ``smoothed``: set by
    ``merge_tets(smooth=n)``; ``v`` then holds the smoothed vertices, ``faces`` and ``closed`` are untouched."""
    v: torch.Tensor                # float32 [Nv, 3]
    faces: torch.Tensor            # int32 [Nt, 3], normals point from inside to outside
    closed: bool
    inside_fraction: float
    grid: int
    bounds: tuple
    level: float
    fill: str = "none"
    cavities: int = 0
    cavity_nodes: int = 0
    islands: int = 0
    island_nodes: int = 0
    smoothed: Optional["SmoothedSurface"] = None          # tssplat_amd.smooth.SmoothedSurface
    simplified: Optional["SimplifiedSurface"] = None      # tssplat_amd.simplify.SimplifiedSurface


@dataclasses.dataclass
class FilledField:
    """``field``: float32 ``[G, G, G]``, a new tensor.  ``cavities``: outside components not touching the grid's border, with
    ``cavity_nodes`` nodes, all of which became inside; ``islands``: solid components dropped by ``"outer"``, with ``island_nodes``."""
    field: torch.Tensor
    cavities: int
    cavity_nodes: int
    islands: int
    island_nodes: int


# ---- argument checks: the shared ones live in tssplat_amd/_args.py; here are the order and what only this module checks ----
_fail = functools.partial(_args.fail, "merge")


def _check_level(name: str, level) -> float:
    """The float32 the kernels compare with, as a Python float."""
    try:
        level = float(np.float32(level))
    except (TypeError, ValueError):
        level = math.nan
    if math.isnan(level):
        _fail(name, "level must be a number, not NaN")
    return level


def _tensor(name: str, arg: str, t, dtype, device=None) -> torch.Tensor:
    """On a GPU, of ``dtype``, on ``device``; a tensor that is not contiguous is copied."""
    return _args.gpu_tensor(_fail, name, arg, t, dtype, device).contiguous()


def _check_mesh(name: str, tet_v, elem):
    tet_v = _tensor(name, "tet_v", tet_v, torch.float32)
    _args.rows(_fail, name, "tet_v", tet_v, 3, math.inf, "[V, 3]")
    elem = _tensor(name, "elem", elem, torch.int32, tet_v.device)
    _args.rows(_fail, name, "elem", elem, 4, _MAX_TETS, "[T, 4] with T <= 2^30")
    return tet_v, elem


def _check_field(name: str, field) -> torch.Tensor:
    field = _tensor(name, "field", field, torch.float32)
    if field.dim() != 3 or not (field.shape[0] == field.shape[1] == field.shape[2]) or not MIN_GRID <= field.shape[0] <= MAX_GRID:
        _fail(name, f"field must be [G, G, G] with G in {MIN_GRID} .. {MAX_GRID}, got {tuple(field.shape)}")
    return field


def _check_fill(name: str, mode, allow_none: bool) -> str:
    return _args.choice(_fail, name, "fill" if allow_none else "mode", mode, (("none",) if allow_none else ()) + tuple(FILL_MODES))


def _check_status(name: str, status: int) -> None:
    if status:
        _fail(name, f"the labelling's {'find walk' if status == 1 else 'union'} ran out of its bound (status {status}): a logic error in "
                    "csrc/fill_kernels.hip, not a property of the field")


def default_level(grid: int, bounds) -> float:
    """``float32(-h 2^-20)``: the surface of the union dilated by a millionth of a voxel.  A node lying on, or within rounding of, a
    face shared by two tets inside the solid reads <= 0 from both; at level 0 it would open a spurious cavity (sphere centres
    from ``init_spheres`` sit on voxel centres, so it happens in practice)."""
    grid = _args.integer(_fail, "default_level", "grid", grid, MIN_GRID, MAX_GRID)
    lo, hi = _args.bounds(_fail, "default_level", bounds)
    return float(np.float32(-((hi - lo) / grid) * 2.0 ** -20))


def default_bounds(tet_v: torch.Tensor, grid: int):
    """``(lo, hi)``: the smallest cube ``[lo, hi]^3`` around all finite coordinates that keeps two nodes (``2 h``) of margin on every
    side.  The grid's cube has ONE interval for all three axes, so it is centred on the interval ``[mn, mx]`` of all finite
    coordinates: ``c = (mn + mx) / 2``, ``E = mx - mn``, ``W = E / (1 - 4 / G)``, ``lo = c - W / 2``, ``hi = c + W / 2`` in float64.
    Needs ``G >= 5`` and ``E > 0``.  One readback of two numbers."""
    name = "default_bounds"
    grid = _args.integer(_fail, name, "grid", grid, 5, MAX_GRID)
    tet_v = _tensor(name, "tet_v", tet_v, torch.float32)
    x = tet_v.reshape(-1)
    x = x[torch.isfinite(x)]
    if x.numel() == 0:
        _fail(name, "tet_v holds no finite coordinate")
    mn, mx = (float(t) for t in torch.stack([x.min(), x.max()]).cpu().numpy().astype(np.float64))
    if not mx > mn:
        _fail(name, "tet_v spans no interval: every finite coordinate is the same")
    c = (mn + mx) / 2.0
    W = (mx - mn) / (1.0 - 4.0 / grid)
    return c - W / 2.0, c + W / 2.0


def _union_field(name, tet_v, elem, grid, lo, hi) -> torch.Tensor:
    lib, ctx, stream = _args.lib_and_stream(tet_v.device)
    field = torch.empty((grid, grid, grid), dtype=torch.float32, device=tet_v.device)
    with ctx:
        _capi.check(lib.tsamd_union_field(_args.ptr(tet_v), int(tet_v.shape[0]), _args.ptr(elem), int(elem.shape[0]), grid, lo, hi, field.data_ptr(), stream))
    return field


def union_field(tet_v: torch.Tensor, elem: torch.Tensor, grid: int, bounds) -> torch.Tensor:
    """float32 ``[G, G, G]``: ``f(p) = max_t min_i dist_i(p)``, the distance to the nearest face plane of the deepest tet around ``p``
    -- positive inside the union, negative outside, ``-inf`` where no tet's bounding box (dilated by one node) holds the node.
    ``tet_v`` float32 ``[V, 3]``, ``elem`` int32 ``[T, 4]``.  A tet contributes only with indices in ``[0, V)``, finite coordinates
    and a positive signed volume ``(b - a) . ((c - a) x (d - a))``: inverted and degenerate tets contribute nothing."""
    name = "union_field"
    tet_v, elem = _check_mesh(name, tet_v, elem)
    grid = _args.integer(_fail, name, "grid", grid, MIN_GRID, MAX_GRID)
    lo, hi = _args.bounds(_fail, name, bounds)
    return _union_field(name, tet_v, elem, grid, lo, hi)


def _count(field, level):
    """(vmask, vcount, tcount, flag): the count phase, enqueued; nothing synchronises."""
    G = int(field.shape[0])
    dev = field.device
    lib, ctx, stream = _args.lib_and_stream(dev)
    n = G * G * G
    vmask, vcount, tcount = (torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(3))
    flag = torch.empty(1, dtype=torch.int32, device=dev)
    with ctx:
        _capi.check(lib.tsamd_surface_count(field.data_ptr(), G, level, vmask.data_ptr(), vcount.data_ptr(), tcount.data_ptr(), flag.data_ptr(), stream))
    return vmask, vcount, tcount, flag


def _emit(field, lo, hi, level, vmask, voffset, toffset, nv, nt):
    """(v, faces): the emit phase, enqueued."""
    G = int(field.shape[0])
    dev = field.device
    lib, ctx, stream = _args.lib_and_stream(dev)
    v = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((nt, 3), dtype=torch.int32, device=dev)
    with ctx:
        _capi.check(lib.tsamd_surface_emit(field.data_ptr(), G, lo, hi, level, vmask.data_ptr(), voffset.data_ptr(), toffset.data_ptr(), nv, nt, _args.ptr(v),
                                           _args.ptr(faces), stream))
    return v, faces


def _extract(field, lo, hi, level):
    """(v, faces, closed): the count phase, two scans, one readback of the totals and the border flag, the emit phase."""
    vmask, vcount, tcount, flag = _count(field, level)
    vscan = torch.cumsum(vcount, 0, dtype=torch.int32)
    tscan = torch.cumsum(tcount, 0, dtype=torch.int32)
    nv, nt, is_open = (int(x) for x in torch.stack([vscan[-1], tscan[-1], flag[0]]).cpu().numpy())      # the one readback
    v, faces = _emit(field, lo, hi, level, vmask, vscan - vcount, tscan - tcount, nv, nt)
    return v, faces, not is_open


def extract_surface(field: torch.Tensor, bounds, level: float):
    """``(v float32 [Nv, 3], faces int32 [Nt, 3], closed)``: marching tetrahedra on the six Kuhn tets of every cube of neighbouring
    nodes (the decomposition of ``scenes.kuhn_ball``: translation-invariant, so neighbouring cubes agree on every face
    diagonal).  A node is inside iff ``field > level`` (a NaN is outside).  Vertices are shared: one per grid edge, face diagonal or
    body diagonal whose ends differ in sign, linearly interpolated in float64.  Triangles are wound from the tets' permutation
    parity so that normals point from inside to outside; a vertex that falls on a node (``f_b == level``) makes degenerate
    triangles.  ``closed``: no node on the grid's border is inside."""
    name = "extract_surface"
    field = _check_field(name, field)
    lo, hi = _args.bounds(_fail, name, bounds)
    return _extract(field, lo, hi, _check_level(name, level))


def occupancy(field: torch.Tensor, level: float) -> torch.Tensor:
    """bool ``[G, G, G]``: ``field > level``, the inside nodes (a NaN is outside)."""
    field = _check_field("occupancy", field)
    return field > _check_level("occupancy", level)


def components(field: torch.Tensor, level: float) -> torch.Tensor:
    """int32 ``[G, G, G]``: per node the smallest flat index ``(i G + j) G + k`` in its component -- a maximal set of nodes with
    equal inside bit (``field > level``; a NaN is outside) connected through the extraction's edges, node +- (di, dj, dk) with
    (di, dj, dk) in {0, 1}^3 without 0.  Inside and outside nodes are labelled in one pass; ``label <= index`` and
    ``label[label] == label``.  One readback: the status word of the bounded device loops."""
    name = "components"
    field = _check_field(name, field)
    level = _check_level(name, level)
    G = int(field.shape[0])
    lib, ctx, stream = _args.lib_and_stream(field.device)
    label = torch.empty((G, G, G), dtype=torch.int32, device=field.device)
    status = torch.empty(1, dtype=torch.int32, device=field.device)
    with ctx:
        _capi.check(lib.tsamd_grid_components(field.data_ptr(), G, level, label.data_ptr(), status.data_ptr(), stream))
    _check_status(name, int(status.cpu()[0]))
    return label


def _fill(name, field, level, mode) -> FilledField:
    """The fill, enqueued, and its one readback: the status word and the four counts together."""
    G = int(field.shape[0])
    dev = field.device
    lib, ctx, stream = _args.lib_and_stream(dev)
    out = torch.empty_like(field)
    workspace = torch.empty(2 * G ** 3 + 2, dtype=torch.int32, device=dev)
    stats = torch.empty(5, dtype=torch.int32, device=dev)
    with ctx:
        _capi.check(lib.tsamd_field_fill(field.data_ptr(), G, level, FILL_MODES[mode], workspace.data_ptr(), out.data_ptr(), stats.data_ptr(), stream))
    status, cavities, cavity_nodes, islands, island_nodes = (int(x) for x in stats.cpu().numpy())
    _check_status(name, status)
    return FilledField(out, cavities, cavity_nodes, islands, island_nodes)


def fill_field(field: torch.Tensor, level: float, mode: str) -> FilledField:
    """The exterior is every outside component that holds a node of the grid's border.  ``mode="cavities"``: every node that is not
    exterior is solid -- enclosed outside components become inside, and an island floating in one merges into the solid.
    ``mode="outer"``: of that solid only the component with the most nodes stays (ties: the smaller label).  In the new field a
    node whose inside bit is unchanged keeps its value bit for bit, an outside node that became inside reads ``+inf`` and an inside
    node that became outside ``-inf``; neither is ever interpolated, because a changed node has no neighbour of opposite final
    sign.  The input is not modified.  One readback."""
    name = "fill_field"
    field = _check_field(name, field)
    level = _check_level(name, level)
    return _fill(name, field, level, _check_fill(name, mode, allow_none=False))


def volume_iou(a: torch.Tensor, b: torch.Tensor) -> float:
    """Intersection over union of two boolean grids of one shape, from two integer counts: exact.  1.0 when both are empty."""
    for arg, t in (("a", a), ("b", b)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.bool:
            _fail("volume_iou", f"{arg} must be a bool tensor")
    if a.shape != b.shape or a.device != b.device:
        _fail("volume_iou", f"b must have a's shape and device ({tuple(a.shape)}, {a.device}), got {tuple(b.shape)}, {b.device}")
    inter, union = (int(x) for x in torch.stack([(a & b).sum(), (a | b).sum()]).cpu().numpy())
    return iou_of_counts(inter, union)


def iou_of_counts(inter: int, union: int) -> float:
    """What :func:`volume_iou` makes of its two counts (``voxelize.mesh_volume_iou`` reads them back with its own)."""
    return inter / union if union else 1.0


def _check_simplify(name: str, simplify, grid: int):
    """``None``, or the integer factor k with 2 <= k <= grid (so that ``grid // k >= 1``)."""
    if simplify is None:
        return None
    if not _args.is_int(simplify, 2, grid):
        _fail(name, f"simplify must be None or an integer in 2 .. grid = {grid}, got {simplify!r}")
    return int(simplify)


def _check_smooth(name: str, smooth):
    """``None``, or the iterations of the default mode: an integer >= 1 (at most ``tssplat_amd.smooth.MAX_ITERATIONS``)."""
    if smooth is None:
        return None
    if not _args.is_int(smooth, 1, 4096):
        _fail(name, f"smooth must be None or an integer in 1 .. 4096, got {smooth!r}")
    return int(smooth)


def merge_tets(tet_v: torch.Tensor, elem: torch.Tensor, grid: int = 128, bounds=None, level=None, fill: str = "none", simplify=None,
               smooth=None) -> MergedSurface:
    """The union of all contributing tets as one closed, consistently oriented triangle mesh: ``union_field`` then
    ``extract_surface``.  ``bounds=None``: :func:`default_bounds`; ``level=None``: :func:`default_level`.  ``fill``: ``"none"`` extracts
    the union field as it is (one closed surface per boundary between components); ``"cavities"`` and ``"outer"`` extract
    :func:`fill_field` of it, at the price of one more readback.  ``simplify=k`` (an integer >= 2): the extracted surface is clustered
    on ``grid // k`` cells per axis over the same bounds (:func:`tssplat_amd.simplify.simplify`, after the fill); ``v`` / ``faces`` / ``closed``
    then describe the clustered mesh and ``simplified`` holds its record.  ``smooth=n`` (an integer >= 1): ``n`` iterations of
    :func:`tssplat_amd.smooth.smooth` with its defaults on the surface that is handed out, last of all; ``v`` then holds the smoothed
    vertices, ``smoothed`` the record, and ``faces`` and ``closed`` are as without."""
    name = "merge_tets"
    fill = _check_fill(name, fill, allow_none=True)
    smooth = _check_smooth(name, smooth)
    tet_v, elem = _check_mesh(name, tet_v, elem)
    grid = _args.integer(_fail, name, "grid", grid, MIN_GRID, MAX_GRID)
    simplify = _check_simplify(name, simplify, grid)
    lo, hi = default_bounds(tet_v, grid) if bounds is None else _args.bounds(_fail, name, bounds)
    level = default_level(grid, (lo, hi)) if level is None else _check_level(name, level)
    field = _union_field(name, tet_v, elem, grid, lo, hi)
    counts = ()
    if fill != "none":
        filled = _fill(name, field, level, fill)
        field, counts = filled.field, (fill, filled.cavities, filled.cavity_nodes, filled.islands, filled.island_nodes)
    v, faces, closed = _extract(field, lo, hi, level)
    n_inside = int((field > level).sum())
    merged = MergedSurface(v, faces, closed, n_inside / float(grid ** 3), grid, (lo, hi), level, *counts)
    if simplify is not None:
        from . import simplify as _simplify
        merged.simplified = _simplify.simplify(v, faces, grid // simplify, (lo, hi))
        merged.v, merged.faces = merged.simplified.v, merged.simplified.faces
        merged.closed = _simplify.edge_stats(merged.faces).closed
    if smooth is not None:
        from . import smooth as _smooth
        merged.smoothed = _smooth.smooth(merged.v, merged.faces, iterations=smooth)
        merged.v = merged.smoothed.v
    return merged


def write_obj(path: str, v, faces) -> None:
    """A plain Wavefront OBJ: ``v x y z`` lines (9 significant digits: float32 reads back exactly) and 1-based ``f a b c`` lines."""
    v = (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).astype(np.float32).reshape(-1, 3)
    f = (faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else np.asarray(faces)).astype(np.int64).reshape(-1, 3) + 1
    lines = ["v %.9g %.9g %.9g" % tuple(p) for p in v.tolist()] + ["f %d %d %d" % tuple(t) for t in f.tolist()]
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + ("\n" if lines else ""))
