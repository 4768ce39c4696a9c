"""Mesh quality on the device: does a triangle surface intersect itself, is it manifold at its edges and at its vertices, how many
pieces has it, is it consistently oriented, and how good are its triangles.

Self-intersection is decided on integers.  Vertices snap to a 2^20 lattice over the cube ``[lo, hi]^3`` (``X = floor((double(x) - lo)
(2^20 - 1) / (hi - lo) + 0.5)``, per vertex, so shared vertices stay shared), and the mesh tested is the SNAPPED mesh: every coordinate
moves by at most 2^-21 of the cube's edge.  ``orient(a, b, c, d) = det(b - a, c - a, d - a)`` in int64; a segment pierces a triangle iff
its ends lie strictly on opposite sides of the triangle's plane and the three edge determinants have one strict sign; valid,
non-degenerate triangles ``i < j`` are a crossing pair iff an edge of one pierces the other.  The kernels sit behind
``tsamd_quality_*`` (include/tssplat_amd.h); tests/quality_oracle.py is the same statement in numpy and the definition.  Integers
only, so the results are bitwise repeatable.  There is no CPU fallback.

Limits.  Strict signs mean that neighbours need no special case (every contact of neighbours has a zero among its signs), and that
these are NOT counted: contacts through a vertex, contacts along an edge, coplanar overlaps, and a crossing whose piercings all pass
exactly through edges of the other triangle.  A triangle that the snap makes degenerate is counted as degenerate and never crosses.

The pair search is brute force with a lattice-box reject.  ``order="morton"`` sorts the triangles by the Morton code of their box
centre (keys from the device, the order from ``torch.sort``) and skips whole tiles whose box misses a wave's; ``order="none"`` visits
every tile and is the statement the other must equal.  The order decides which pairs are evaluated, never the result: ``crossings``,
the sorted ``pairs`` and every count are equal, byte for byte (``box_pairs`` too: a skipped tile holds no box that overlaps); only
``tile_visits``, the cost, differs.

Topology is counted over the valid triangles, with the edge keys sorted by ``torch.sort`` as :func:`tssplat_amd.simplify.edge_stats`
has it and two device union-finds: vertices joined by edges (``component``), and the corners at a vertex joined through shared edges
(``fans``).  :func:`topology` synchronises the host once per union-find round.

Out of scope: counting touching and coplanar contacts; repairing anything (removing crossings, splitting non-manifold vertices,
reorienting); a tree or grid beyond the tile boxes; tet-mesh quality.
"""
from __future__ import annotations

import ctypes
import dataclasses
import functools
import math

import numpy as np
import torch

from . import _args, _capi

__all__ = ["SelfIntersections", "Topology", "Shape", "MeshQuality", "self_intersections", "topology", "shape", "mesh_quality", "launch_info",
           "MAX_TRIANGLES", "MAX_PAIRS", "ORDERS", "DEFAULT_ORDER", "LATTICE"]

LATTICE = 1 << 20
MAX_TRIANGLES = 2 ** 31 // 3 - 1          # corner ids 3 t + k are 32-bit (include/tssplat_amd.h)
MAX_PAIRS = 2 ** 31 - 1
ORDERS = ("none", "morton")
DEFAULT_ORDER = "morton"
_SENTINEL = 2 ** 63 - 1
# the words of the stats record: the header's TSAMD_QUALITY_* names in value order ("crossing_pairs", ..., "tile_visits")
_STATS = tuple(name[len("TSAMD_QUALITY_"):].lower()
               for name in sorted((n for n in _capi.HEADER.constants if n.startswith("TSAMD_QUALITY_")), key=_capi.HEADER.constants.get))


@dataclasses.dataclass
class SelfIntersections:
    """``crossings`` int32 ``[T]``: the crossing pairs each triangle is in.  ``pairs`` int64 ``[crossing_pairs]``: the keys ``i << 32 | j``,
    ``i < j``, ascending -- or ``None`` with ``pairs_truncated`` when there are more than ``max_pairs`` (an overfull list's content
    depends on timing and is not handed out).  ``box_pairs``: pairs that passed the box reject."""
    crossings: torch.Tensor
    pairs: torch.Tensor | None
    pairs_truncated: bool
    crossing_pairs: int
    crossing_faces: int
    invalid_faces: int
    degenerate_faces: int
    box_pairs: int
    tile_visits: int
    bounds: tuple
    order: str


@dataclasses.dataclass
class Topology:
    """Counts over the valid triangles.  ``component`` int32 ``[Nv]``: the lowest vertex index of the vertex's component, -1 for a vertex no
    valid triangle uses.  ``fans`` int32 ``[Nv]``: the classes of the corners at the vertex (1 on a manifold surface)."""
    edges: int
    boundary_edges: int
    nonmanifold_edges: int
    repeated_directed_edges: int
    oriented: bool
    components: int
    component: torch.Tensor
    fans: torch.Tensor
    nonmanifold_vertices: int
    manifold: bool
    euler: int
    closed: bool
    valid_faces: int
    referenced_vertices: int
    union_rounds: tuple


@dataclasses.dataclass
class Shape:
    """``alr = 12 sqrt(3) A / P^2`` per valid triangle (1 equilateral, 0 degenerate) and the minimum angle in degrees."""
    faces: int
    alr_mean: float
    alr_min: float
    alr_p05: float
    alr_below_0p1: float
    min_angle_min: float
    min_angle_mean: float


@dataclasses.dataclass
class MeshQuality:
    intersections: SelfIntersections
    topology: Topology
    shape: Shape
    watertight: bool

    def as_dict(self) -> dict:
        """Every figure, without the per-triangle and per-vertex tensors: what a JSON record holds."""
        flat = lambda r: {f.name: getattr(r, f.name) for f in dataclasses.fields(r) if not isinstance(getattr(r, f.name), torch.Tensor)}   # noqa: E731
        si = flat(self.intersections)
        si.pop("pairs", None)
        return {"watertight": self.watertight, "intersections": si, "topology": flat(self.topology), "shape": flat(self.shape)}


# ---- argument checks: the shared ones live in tssplat_amd/_args.py; here are the order and what only this module checks ----
_fail = functools.partial(_args.fail, "quality")
_ptr = _args.ptr


def _check_mesh(name: str, v, faces):
    v, faces = _args.triangle_mesh(_fail, name, v, faces, MAX_TRIANGLES)
    return v.contiguous(), faces.contiguous()


def _bounds(name: str, v, faces, bounds):
    """The cube: the caller's, or simplify's min / max over the finite coordinates (one readback); a mesh with nothing to span gets the
    unit cube, under which it has no valid triangle with an extent anyway."""
    if bounds is not None:
        return bounds
    if int(faces.shape[0]) == 0 or int(v.shape[0]) == 0:
        return 0.0, 1.0
    x = v.reshape(-1)
    x = x[torch.isfinite(x)]
    if x.numel() == 0:
        return 0.0, 1.0
    lo, hi = (float(t) for t in torch.stack(torch.aminmax(x)).cpu().numpy().astype(np.float64))
    if not hi > lo:
        return lo - 0.5, lo + 0.5
    return _args.bounds(_fail, name, (lo, hi))


def launch_info() -> dict:
    """The compiled launch constants: triangles per workgroup (Q), triangles per LDS tile (K), queue entries per wave."""
    lib = _capi.load()
    q, k, n = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    _capi.check(lib.tsamd_quality_info(ctypes.byref(q), ctypes.byref(k), ctypes.byref(n)))
    return {"block": q.value, "tile": k.value, "queue": n.value}


def _prepare(v, faces, lo, hi):
    """(corners, boxes, state, shape, morton), enqueued."""
    dev = v.device
    T = int(faces.shape[0])
    lib, ctx, stream = _args.lib_and_stream(dev)
    corners = torch.empty((T, 3), dtype=torch.int64, device=dev)
    boxes = torch.empty((T, 2), dtype=torch.int64, device=dev)
    state = torch.empty(T, dtype=torch.uint8, device=dev)
    rec = torch.empty((T, 4), dtype=torch.float64, device=dev)
    morton = torch.empty(T, dtype=torch.int64, device=dev)
    with ctx:
        _capi.check(lib.tsamd_quality_prepare(_ptr(v), int(v.shape[0]), _ptr(faces), T, lo, hi, _ptr(corners), _ptr(boxes), _ptr(state), _ptr(rec), _ptr(morton),
                                              stream))
    return corners, boxes, state, rec, morton


def _pairs(corners, boxes, state, max_pairs, skip_tiles):
    dev = corners.device
    T = int(corners.shape[0])
    lib, ctx, stream = _args.lib_and_stream(dev)
    crossings = torch.empty(T, dtype=torch.int32, device=dev)
    pairs = torch.empty(max_pairs, dtype=torch.int64, device=dev)
    stats = torch.empty(8, dtype=torch.int64, device=dev)
    tile_boxes = torch.empty((-(-T // launch_info()["tile"]), 2), dtype=torch.int64, device=dev) if skip_tiles else None
    with ctx:
        _capi.check(lib.tsamd_quality_pairs(_ptr(corners), _ptr(boxes), _ptr(state), T, None if tile_boxes is None else _ptr(tile_boxes), max_pairs,
                                            _ptr(crossings), _ptr(pairs), stats.data_ptr(), stream))
    return crossings, pairs, stats


def _self_intersections(prepared, lo, hi, max_pairs, order) -> SelfIntersections:
    corners, boxes, state, _, morton = prepared
    dev = corners.device
    T = int(corners.shape[0])
    if T == 0:
        return SelfIntersections(torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int64, device=dev), False, 0, 0, 0, 0, 0, 0,
                                 (lo, hi), order)
    perm = None
    if order == "morton":
        perm = torch.sort(morton)[1]                                    # ties in any order: the order never decides a result
        corners, boxes, state = corners[perm].contiguous(), boxes[perm].contiguous(), state[perm].contiguous()
    crossings, pairs, stats = _pairs(corners, boxes, state, max_pairs, perm is not None)
    s = dict(zip(_STATS, (int(x) for x in stats.cpu().numpy()[:len(_STATS)])))           # the one readback
    if perm is not None:
        crossings = torch.zeros_like(crossings).scatter_(0, perm, crossings)
    truncated = s["crossing_pairs"] > max_pairs
    out = None
    if not truncated:
        keys = pairs[:s["crossing_pairs"]]
        if perm is not None:
            i, j = perm[keys >> 32], perm[keys & 0xFFFFFFFF]
            keys = (torch.minimum(i, j) << 32) | torch.maximum(i, j)
        out = torch.sort(keys)[0]
    return SelfIntersections(crossings, out, truncated, s["crossing_pairs"], s["crossing_faces"], s["invalid_faces"], s["degenerate_faces"], s["box_pairs"],
                             s["tile_visits"], (lo, hi), order)


def _union(pairs, n, dev):
    lib, ctx, stream = _args.lib_and_stream(dev)
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    flag = torch.empty(1, dtype=torch.int32, device=dev)
    rounds = ctypes.c_int64()
    with ctx:
        _capi.check(lib.tsamd_quality_union(_ptr(pairs), int(pairs.shape[0]) if pairs.numel() else 0, _ptr(labels), n, flag.data_ptr(), ctypes.byref(rounds), stream))
    return labels, int(rounds.value)


def _topology(faces, state, n_vertices) -> Topology:
    dev = faces.device
    T, Nv = int(faces.shape[0]), int(n_vertices)
    if T == 0:
        return Topology(0, 0, 0, 0, True, 0, torch.full((Nv,), -1, dtype=torch.int32, device=dev), torch.zeros(Nv, dtype=torch.int32, device=dev), 0, True, 0,
                        True, 0, 0, (0, 0))
    lib, ctx, stream = _args.lib_and_stream(dev)
    und = torch.empty(3 * T, dtype=torch.int64, device=dev)
    directed = torch.empty(3 * T, dtype=torch.int64, device=dev)
    vpairs = torch.empty((3 * T, 2), dtype=torch.int32, device=dev)
    referenced = torch.empty(Nv, dtype=torch.uint8, device=dev)
    with ctx:
        _capi.check(lib.tsamd_quality_edges(_ptr(faces), _ptr(state), T, Nv, _ptr(und), _ptr(directed), _ptr(vpairs), _ptr(referenced), stream))
    keys, order = torch.sort(und)
    cpairs = torch.empty((3 * T, 2, 2), dtype=torch.int32, device=dev)
    with ctx:
        _capi.check(lib.tsamd_quality_fan_pairs(_ptr(faces), T, _ptr(keys), _ptr(order), _ptr(cpairs), stream))
    vlabel, rounds_v = _union(vpairs, Nv, dev) if Nv else (torch.zeros(0, dtype=torch.int32, device=dev), 0)
    clabel, rounds_c = _union(cpairs.reshape(-1, 2), 3 * T, dev)
    used = referenced != 0
    component = torch.where(used, vlabel, torch.full_like(vlabel, -1))
    valid_corner = (state != 2).repeat_interleave(3)
    root = valid_corner & (clabel == torch.arange(3 * T, dtype=torch.int32, device=dev))
    fans = torch.bincount(faces.reshape(-1)[root].long(), minlength=Nv).to(torch.int32) if Nv else torch.zeros(0, dtype=torch.int32, device=dev)
    live = keys[keys != _SENTINEL]
    counts = torch.unique_consecutive(live, return_counts=True)[1]
    dsorted = torch.sort(directed)[0]
    distinct = torch.unique_consecutive(dsorted[dsorted != _SENTINEL])
    vidx = torch.arange(Nv, dtype=torch.int32, device=dev)
    figures = torch.stack([(counts > 0).sum(), (counts == 1).sum(), (counts > 2).sum(), (counts == 2).sum(), torch.tensor(live.shape[0], device=dev),
                           torch.tensor(distinct.shape[0], device=dev), (used & (vlabel == vidx)).sum(), (fans > 1).sum(), used.sum(), (state != 2).sum()])
    edges, boundary, nonmanifold, two, n_directed, n_distinct, components, nmv, n_ref, n_valid = (int(x) for x in figures.cpu().numpy())   # the one readback
    repeated = n_directed - n_distinct
    return Topology(edges, boundary, nonmanifold, repeated, repeated == 0, components, component, fans, nmv, nonmanifold == 0 and nmv == 0,
                    n_ref - edges + n_valid, bool(two == edges and repeated == 0), n_valid, n_ref, (rounds_v, rounds_c))


def _shape(rec) -> Shape:
    """Float64 torch on the per-triangle record: plumbing."""
    s = rec[torch.isfinite(rec).all(1)]
    n = int(s.shape[0])
    if n == 0:
        return Shape(0, math.nan, math.nan, math.nan, math.nan, math.nan, math.nan)
    per = torch.sqrt(s[:, :3]).sum(1)
    area = 0.5 * torch.sqrt(s[:, 3])
    alr = torch.where(per > 0, 12.0 * math.sqrt(3.0) * area / (per * per), torch.zeros_like(per))
    k = torch.argmin(s[:, :3], 1, keepdim=True)
    e0 = torch.gather(s[:, :3], 1, k)[:, 0]
    others = s[:, :3].sum(1) - e0
    angle = torch.rad2deg(torch.atan2(torch.sqrt(s[:, 3]), 0.5 * (others - e0)))        # opposite the shortest edge
    angle = torch.where(torch.isfinite(angle), angle, torch.zeros_like(angle))
    p05 = torch.sort(alr)[0][min(n - 1, int(math.floor(0.05 * (n - 1))))]
    out = torch.stack([alr.mean(), alr.min(), p05, (alr < 0.1).double().mean(), angle.min(), angle.mean()]).cpu().numpy()   # the one readback
    return Shape(n, *(float(x) for x in out))


# ---- the public interface ----
def self_intersections(v: torch.Tensor, faces: torch.Tensor, bounds=None, max_pairs: int = 65536, order: str = DEFAULT_ORDER) -> SelfIntersections:
    """The crossing pairs of the mesh ``v`` float32 ``[Nv, 3]``, ``faces`` int32 ``[T, 3]`` snapped to the 2^20 lattice over ``bounds = (lo, hi)``,
    one interval for all three axes; ``bounds=None``: the min / max over all finite coordinates as :func:`tssplat_amd.simplify.simplify`
    takes it (one more readback).  A triangle with a vertex outside the cube is invalid.  ``max_pairs``: the capacity of the pair list.
    See the module text for what is and is not counted."""
    name = "self_intersections"
    max_pairs = _args.integer(_fail, name, "max_pairs", max_pairs, 0, MAX_PAIRS)
    order = _args.choice(_fail, name, "order", order, ORDERS)
    if bounds is not None:
        bounds = _args.bounds(_fail, name, bounds)
    v, faces = _check_mesh(name, v, faces)
    lo, hi = _bounds(name, v, faces, bounds)
    return _self_intersections(_prepare(v, faces, lo, hi), lo, hi, max_pairs, order)


def topology(v: torch.Tensor, faces: torch.Tensor, bounds=None) -> Topology:
    """Edge, orientation, component and fan counts over the valid triangles (validity as :func:`self_intersections` has it: under
    ``bounds=None`` every triangle with in-range indices and finite coordinates)."""
    name = "topology"
    if bounds is not None:
        bounds = _args.bounds(_fail, name, bounds)
    v, faces = _check_mesh(name, v, faces)
    lo, hi = _bounds(name, v, faces, bounds)
    return _topology(faces, _prepare(v, faces, lo, hi)[2], int(v.shape[0]))


def shape(v: torch.Tensor, faces: torch.Tensor) -> Shape:
    """Area-length ratio and minimum angle over the triangles with in-range indices and finite coordinates."""
    name = "shape"
    v, faces = _check_mesh(name, v, faces)
    if int(faces.shape[0]) == 0:
        return _shape(torch.zeros((0, 4), dtype=torch.float64, device=v.device))
    lo, hi = _bounds(name, v, faces, None)                              # every triangle with finite coordinates is valid under it
    return _shape(_prepare(v, faces, lo, hi)[3])


def mesh_quality(v: torch.Tensor, faces: torch.Tensor, bounds=None, max_pairs: int = 65536, order: str = DEFAULT_ORDER) -> MeshQuality:
    """All three records from one prepare pass (one readback per part), and ``watertight = closed and manifold and oriented and
    crossing_pairs == 0``."""
    name = "mesh_quality"
    max_pairs = _args.integer(_fail, name, "max_pairs", max_pairs, 0, MAX_PAIRS)
    order = _args.choice(_fail, name, "order", order, ORDERS)
    if bounds is not None:
        bounds = _args.bounds(_fail, name, bounds)
    v, faces = _check_mesh(name, v, faces)
    lo, hi = _bounds(name, v, faces, bounds)
    prepared = _prepare(v, faces, lo, hi)
    si = _self_intersections(prepared, lo, hi, max_pairs, order)
    topo = _topology(faces, prepared[2], int(v.shape[0]))
    sh = _shape(prepared[3])
    return MeshQuality(si, topo, sh, bool(topo.closed and topo.manifold and topo.oriented and si.crossing_pairs == 0))
