"""Simplifying a triangle surface on the device: vertex clustering on a cube grid with quadric placement.

Every vertex falls into one cell of a ``cells``^3 grid; all vertices of a cell become ONE vertex, placed where the summed plane
quadrics of the triangles touching the cell are smallest (Rossignac-Borrel's clustering with Lindstrom's area^2-weighted quadrics
and a Tikhonov pull towards the cell's mean vertex, as DeCoro-Tatarchuk run it on a GPU), and a triangle survives iff its corners
fall into three different cells.  The grid is the merge's: one interval ``[lo, hi]`` for all three axes, ``h = (hi - lo) / cells``.
The kernels sit behind ``tsamd_simplify_keys``, ``_cells``, ``_faces`` and ``_dedupe`` (include/tssplat_amd.h), stated in separately
rounded float64 operations, sequential per-cell sums and integers, so the result is bitwise repeatable; tests/simplify_oracle.py
is the same statement in numpy and the definition.  There is no CPU fallback.

Limits.  Clustering does NOT preserve manifoldness: two sheets of the surface passing through one cell are welded, and a thin
handle can collapse to an edge.  :func:`edge_stats` reports what came out; ``closed`` is reported, never promised.  A cell's records
are summed serially by one lane, so a grid with very few cells on a large mesh (``cells=1`` at the extreme) is slow by construction.

Out of scope: edge collapses, manifold repair, re-tetrahedralising.  Smoothing is :mod:`tssplat_amd.smooth`.
"""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np
import torch

from . import _args, _capi

__all__ = ["SimplifiedSurface", "EdgeStats", "simplify", "edge_stats", "run_lengths", "MAX_CELLS", "MAX_TRIANGLES", "PLACEMENTS", "DEFAULT_STABILISE"]

MAX_CELLS = 1024                          # cell keys stay below 2^30
MAX_TRIANGLES = (2 ** 31 - 1) // 3        # three record slots per triangle, indexed with 32 bits (include/tssplat_amd.h)
PLACEMENTS = {"quadric": _capi.TSAMD_SIMPLIFY_QUADRIC, "mean": _capi.TSAMD_SIMPLIFY_MEAN}    # include/tssplat_amd.h
DEFAULT_STABILISE = 2.0 ** -10
_SENTINEL = 2 ** 63 - 1


@dataclasses.dataclass
class SimplifiedSurface:
    """``v`` / ``faces``: the clustered mesh, vertices in ascending cell-key order, faces in input order.  ``cells_occupied``: cells that hold
    a vertex of a valid face; ``clamped``: those whose representative had to be clamped into its cell; ``duplicates``: surviving faces
    dropped because an earlier face had the same three cells in the same orientation; ``degenerate_faces``: valid faces whose corners
    share a cell; ``invalid_faces``: faces with an index outside the vertices or a vertex that is not finite."""
    v: torch.Tensor                  # float32 [Nv', 3]
    faces: torch.Tensor              # int32 [Nt', 3]
    cells: int
    bounds: tuple
    placement: str
    cells_occupied: int
    clamped: int
    duplicates: int
    degenerate_faces: int
    invalid_faces: int


@dataclasses.dataclass
class EdgeStats:
    """``edges``: distinct undirected edges; ``boundary_edges``: those in exactly one triangle; ``nonmanifold_edges``: those in more than two;
    ``closed``: every undirected edge lies in exactly two triangles, once in each direction."""
    edges: int
    boundary_edges: int
    nonmanifold_edges: int
    closed: bool

    def __iter__(self):
        return iter((self.edges, self.boundary_edges, self.nonmanifold_edges, self.closed))


# ---- argument checks: the shared ones live in tssplat_amd/_args.py; here are the order and what only this module checks ----
_fail = functools.partial(_args.fail, "simplify")
_ptr = _args.ptr


def _check_mesh(name: str, v, faces):
    """Types and shapes of both first, then where they live; a tensor that is not contiguous is copied."""
    v, faces = _args.triangle_mesh(_fail, name, v, faces, MAX_TRIANGLES)
    return v.contiguous(), faces.contiguous()


def _check_stabilise(name: str, stabilise) -> float:
    try:
        s = float(stabilise)
    except (TypeError, ValueError):
        s = math.nan
    if isinstance(stabilise, bool) or not (math.isfinite(s) and s >= 0.0):
        _fail(name, f"stabilise must be a finite number >= 0, got {stabilise!r}")
    return s


def _check_status(name: str, status: int) -> None:
    if status:
        _fail(name, f"a device stage met {'records' if status == 1 else 'a face order'} that the stage before cannot have written (status {status}): a logic "
                    "error in csrc/simplify_kernels.hip or in the sorts between its stages, not a property of the mesh")


def _auto_bounds(name: str, v: torch.Tensor):
    """The min / max over all finite coordinates: one aminmax, one readback."""
    x = v.reshape(-1)
    x = x[torch.isfinite(x)]
    if x.numel() == 0:
        _fail(name, "v holds no finite coordinate: bounds=None has nothing to span")
    lo, hi = (float(t) for t in torch.stack(torch.aminmax(x)).cpu().numpy().astype(np.float64))
    if not hi > lo:
        _fail(name, "v spans no interval (every finite coordinate is the same): pass bounds")
    return lo, hi


def _keys(v, faces, cells, lo, hi):
    """(vkey, records, state): the cell keys and the three record slots per face, enqueued."""
    dev = v.device
    Nv, Nt = int(v.shape[0]), int(faces.shape[0])
    lib, ctx, stream = _args.lib_and_stream(dev)
    vkey = torch.empty(Nv, dtype=torch.int32, device=dev)
    records = torch.empty(3 * Nt, dtype=torch.int64, device=dev)
    state = torch.empty(Nt, dtype=torch.uint8, device=dev)
    with ctx:
        _capi.check(lib.tsamd_simplify_keys(_ptr(v), Nv, _ptr(faces), Nt, cells, lo, hi, _ptr(vkey), _ptr(records), _ptr(state), stream))
    return vkey, records, state


def _cells(v, faces, cells, lo, hi, placement, stabilise, vkey, records, perm, status):
    """(pos, head, run): the run walk and the solve over the SORTED records, enqueued."""
    dev = v.device
    S = int(records.shape[0])
    lib, ctx, stream = _args.lib_and_stream(dev)
    pos = torch.empty((S, 3), dtype=torch.float32, device=dev)
    head = torch.empty(S, dtype=torch.uint8, device=dev)
    run = torch.empty(S, dtype=torch.int32, device=dev)
    with ctx:
        _capi.check(lib.tsamd_simplify_cells(_ptr(v), int(v.shape[0]), _ptr(faces), int(faces.shape[0]), cells, lo, hi, PLACEMENTS[placement], stabilise,
                                             _ptr(vkey), _ptr(records), _ptr(perm), _ptr(pos), _ptr(head), _ptr(run), status.data_ptr(), stream))
    return pos, head, run


def _faces(run, state, status):
    """(tri, keep, used): the rotated run triples, the (triple, index) order by two stable sorts, the duplicate flags and used marks."""
    dev = run.device
    Nt = int(state.shape[0])
    lib, ctx, stream = _args.lib_and_stream(dev)
    tri = torch.empty((Nt, 3), dtype=torch.int32, device=dev)
    key_ab = torch.empty(Nt, dtype=torch.int64, device=dev)
    key_c = torch.empty(Nt, dtype=torch.int64, device=dev)
    with ctx:
        _capi.check(lib.tsamd_simplify_faces(_ptr(run), _ptr(state), Nt, _ptr(tri), _ptr(key_ab), _ptr(key_c), stream))
    # by c, then by (a, b): equal keys keep the order they came in, which starts as the index
    by_c = torch.sort(key_c, stable=True)[1]
    order = by_c[torch.sort(key_ab[by_c], stable=True)[1]].contiguous()
    keep = torch.empty(Nt, dtype=torch.uint8, device=dev)
    used = torch.empty(3 * Nt, dtype=torch.uint8, device=dev)
    with ctx:
        _capi.check(lib.tsamd_simplify_dedupe(_ptr(tri), _ptr(order), Nt, _ptr(keep), _ptr(used), status.data_ptr(), stream))
    return tri, keep, used


def _compact(name, pos, head, state, tri, keep, used, status):
    """(v, faces, counts): the one readback (both status words and every count), then the compaction by a scan of the used marks."""
    vscan = torch.cumsum(used, 0, dtype=torch.int32)                    # integers: any scan order gives the same bits
    counts = torch.stack([status[0].long(), status[1].long(), (head != 0).sum(), (head == 3).sum(), (state == 0).sum(), (state == 1).sum(),
                          (state == 2).sum(), keep.sum(dtype=torch.int64)])
    st_cells, st_order, occupied, clamped, survivors, degenerate, invalid, kept = (int(x) for x in counts.cpu().numpy())
    _check_status(name, st_cells or st_order)
    out_v = pos[used != 0].contiguous()
    number = vscan - 1                                                   # a used run's output vertex; runs ascend with the cell key
    out_f = number[tri[keep != 0].long().reshape(-1)].reshape(-1, 3).contiguous()
    return out_v, out_f, (occupied, clamped, survivors - kept, degenerate, invalid)


def _simplify(name, v, faces, cells, lo, hi, placement, stabilise) -> SimplifiedSurface:
    dev = v.device
    if int(faces.shape[0]) == 0:
        return SimplifiedSurface(torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty((0, 3), dtype=torch.int32, device=dev), cells, (lo, hi),
                                 placement, 0, 0, 0, 0, 0)
    status = torch.empty(2, dtype=torch.int32, device=dev)
    vkey, records, state = _keys(v, faces, cells, lo, hi)
    records, perm = torch.sort(records)                                 # unique keys (and equal sentinels, which nobody tells apart)
    pos, head, run = _cells(v, faces, cells, lo, hi, placement, stabilise, vkey, records, perm, status[0:1])
    tri, keep, used = _faces(run, state, status[1:2])
    out_v, out_f, counts = _compact(name, pos, head, state, tri, keep, used, status)
    return SimplifiedSurface(out_v, out_f, cells, (lo, hi), placement, *counts)


def simplify(v: torch.Tensor, faces: torch.Tensor, cells: int, bounds=None, placement: str = "quadric", stabilise: float = DEFAULT_STABILISE) -> SimplifiedSurface:
    """Clusters the mesh ``v`` float32 ``[Nv, 3]``, ``faces`` int32 ``[Nt, 3]`` on ``cells``^3 cells (1 .. 1024) over ``bounds = (lo, hi)``, one interval for
    all three axes as in :mod:`tssplat_amd.merge`; ``bounds=None``: the min / max over all finite coordinates (one more readback).  A
    vertex outside the bounds counts for the border cell next to it.  ``placement``: ``"quadric"`` puts a cell's vertex at the minimum of
    the summed plane quadrics of the triangles touching the cell, regularised by ``stabilise`` times the quadric's trace towards the
    cell's mean vertex (a parameter of the method: it keeps flat and creased cells well-posed) and clamped into the cell;
    ``"mean"`` at the mean vertex.  An empty result (``cells=1``, say) has shapes ``[0, 3]``.  See the module text for what clustering
    does not preserve."""
    name = "simplify"
    cells = _args.integer(_fail, name, "cells", cells, 1, MAX_CELLS)
    placement = _args.choice(_fail, name, "placement", placement, PLACEMENTS)
    stabilise = _check_stabilise(name, stabilise)
    if bounds is not None:
        bounds = _args.bounds(_fail, name, bounds, cells)
    v, faces = _check_mesh(name, v, faces)
    lo, hi = _args.bounds(_fail, name, _auto_bounds(name, v), cells) if bounds is None else bounds
    return _simplify(name, v, faces, cells, lo, hi, placement, stabilise)


def run_lengths(v: torch.Tensor, faces: torch.Tensor, cells: int, bounds=None) -> torch.Tensor:
    """int64 ``[cells_occupied]``: how many records each occupied cell's lane walks, in ascending cell order -- the serial depth of the
    cell stage.  Plain device torch ops on the sorted records."""
    name = "run_lengths"
    cells = _args.integer(_fail, name, "cells", cells, 1, MAX_CELLS)
    if bounds is not None:
        bounds = _args.bounds(_fail, name, bounds, cells)
    v, faces = _check_mesh(name, v, faces)
    lo, hi = _args.bounds(_fail, name, _auto_bounds(name, v), cells) if bounds is None else bounds
    if int(faces.shape[0]) == 0:
        return torch.zeros(0, dtype=torch.int64, device=v.device)
    records = torch.sort(_keys(v, faces, cells, lo, hi)[1])[0]
    return torch.unique_consecutive(records[records != _SENTINEL] >> 32, return_counts=True)[1]


def edge_stats(faces: torch.Tensor) -> EdgeStats:
    """``(edges, boundary_edges, nonmanifold_edges, closed)`` of ``faces`` int32 ``[Nt, 3]`` (indices >= 0): sort and ``unique_consecutive`` of 64-bit
    edge keys on the device, one readback.  No triangle: ``(0, 0, 0, True)``."""
    name = "edge_stats"
    faces = _args.placed(_fail, name, "faces", _args.typed_rows(_fail, name, "faces", faces, torch.int32, MAX_TRIANGLES))    # torch ops only: any layout
    if int(faces.shape[0]) == 0:
        return EdgeStats(0, 0, 0, True)
    f = faces.long()
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
    und = torch.sort((torch.minimum(a, b) << 32) | torch.maximum(a, b))[0]
    counts = torch.unique_consecutive(und, return_counts=True)[1]
    directed = torch.unique_consecutive(torch.sort((a << 32) | b)[0])
    edges, boundary, nonmanifold, two = (int(x) for x in torch.stack([(counts > 0).sum(), (counts == 1).sum(), (counts > 2).sum(), (counts == 2).sum()]).cpu().numpy())
    return EdgeStats(edges, boundary, nonmanifold, bool(two == edges and int(directed.shape[0]) == int(a.shape[0])))
