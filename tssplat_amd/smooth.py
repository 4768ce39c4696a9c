"""Smoothing a triangle surface on the device without touching its faces: Taubin's lambda | mu filter and tangential relaxation.

Smoothing moves vertices and leaves ``faces`` alone, so closedness, manifoldness, components, orientation and the atlas layout all
survive it.  It promises unchanged connectivity; it does NOT promise a surface free of self-intersections --
:func:`tssplat_amd.quality.self_intersections` says what came out.

The operator is the umbrella ``L_i = (sum of p_j over the neighbours N(i), ascending) / deg_i - p_i`` over the valid faces (three
indices in range, pairwise distinct).  ``mode="taubin"``: one iteration is ``p <- p + lam L(p)`` and then ``p <- p + mu L(p)`` on the
result (Taubin 1995: with ``mu < -lam < 0`` a low-pass filter that does not shrink; ``mu = 0`` is the plain Laplacian, which does).
``mode="tangential"``: ``d = lam L_i`` loses its component along the vertex normal ``n_i``, the sum of the cross products of its faces
(Botsch-Kobbelt's relaxation: better triangles, the surface's shape kept to first order).  Positions are held in float64 from
``double(v)`` through all iterations and rounded to float32 once at the end; a state that overflows comes out as an infinity or a
NaN in float32: nothing is special-cased beyond IEEE.  The kernels sit behind ``tsamd_smooth_*`` (include/tssplat_amd.h), stated in
separately rounded float64 operations and sequential sums in ascending row order, so the result is bitwise repeatable;
tests/smooth_oracle.py is the same statement in numpy and the definition.  There is no CPU fallback.

A vertex moves iff it is finite, has a neighbour, all its neighbours are finite in the input, it is not pinned, and
``boundary="free"`` or it lies on no edge that is in some number of valid faces other than two.  Every other vertex comes out with
its input bits.  ``boundary="fixed"`` is the default because the umbrella of a vertex on a boundary or non-manifold edge pulls it
off that edge and folds the triangles next to it.

Limits.  One lane walks a vertex's row (and, tangential, its faces) serially, so a hub vertex of very high degree (the apex of a
fan at the extreme) holds its wave for as long as its row is: slow by construction, never wrong.  Uniform weights pull vertices
towards even spacing, so Taubin smoothing also slides them within the surface.

Out of scope: cotangent or other weights, feature-edge detection, smoothing along boundary curves, anything that changes
``faces``, and repair.
"""
from __future__ import annotations

import ctypes
import dataclasses
import functools
import math
from typing import Optional

import torch

from . import _args, _capi

__all__ = ["VertexAdjacency", "SmoothedSurface", "adjacency", "smooth", "MODES", "DEFAULT_MODE", "BOUNDARIES", "MAX_ITERATIONS", "MAX_TRIANGLES", "STATE_STRIDE"]

MODES = {"taubin": _capi.TSAMD_SMOOTH_TAUBIN, "tangential": _capi.TSAMD_SMOOTH_TANGENTIAL}        # include/tssplat_amd.h
DEFAULT_MODE = "taubin"
BOUNDARIES = {"fixed": _capi.TSAMD_SMOOTH_BOUNDARY_FIXED, "free": _capi.TSAMD_SMOOTH_BOUNDARY_FREE}
MAX_ITERATIONS = 4096
MAX_TRIANGLES = 2 ** 31 // 6 - 1              # six directed keys per face, positions are 32-bit (include/tssplat_amd.h)
STATE_STRIDE = 3                              # float64 per state record: 24 bytes beat the padded 32 on every mesh measured (DESIGN section 19 has both figures)


@dataclasses.dataclass
class VertexAdjacency:
    """The connectivity of the valid faces.  Row ``i`` of ``neighbours`` is ``offsets[i] .. offsets[i + 1]``: the distinct vertices sharing an
    edge with ``i``, ascending; ``faces_of`` under ``face_offsets`` likewise lists the valid faces that contain ``i``.  ``irregular``: 1 for a
    vertex on an edge that is in some number of valid faces other than two (a boundary or non-manifold edge; a face listed twice
    counts twice).  ``valid``: 1 for a face with three distinct indices in range."""
    offsets: torch.Tensor          # int32 [Nv + 1]
    neighbours: torch.Tensor       # int32 [offsets[-1]]
    face_offsets: torch.Tensor     # int32 [Nv + 1]
    faces_of: torch.Tensor         # int32 [3 x valid faces]
    irregular: torch.Tensor        # uint8 [Nv]
    valid: torch.Tensor            # uint8 [Nt]


@dataclasses.dataclass
class SmoothedSurface:
    """``v``: the smoothed vertices; ``faces``: the caller's tensor.  ``moved`` + ``held_other`` + ``held_pinned`` + ``held_irregular`` = Nv, a held
    vertex counted under the first reason that applies in that order; ``held_other``: not finite, a neighbour not finite, or in no
    valid face."""
    v: torch.Tensor                # float32 [Nv, 3]
    faces: torch.Tensor
    iterations: int
    mode: str
    lam: float
    mu: float
    boundary: str
    max_move: Optional[float]
    project: bool
    moved: int
    held_other: int
    held_pinned: int
    held_irregular: int


# ---- argument checks: the shared ones live in tssplat_amd/_args.py; here are the order and what only this module checks ----
_fail = functools.partial(_args.fail, "smooth")
_ptr = _args.ptr


def _check_mesh(name: str, v, faces):
    v, faces = _args.triangle_mesh(_fail, name, v, faces, MAX_TRIANGLES)
    return v.contiguous(), faces.contiguous()


def _number(name: str, arg: str, x, least=None) -> float:
    """A finite float (a bool is no number), ``>= least`` when that is given."""
    try:
        y = float(x)
    except (TypeError, ValueError):
        y = math.nan
    if isinstance(x, bool) or not math.isfinite(y) or (least is not None and y < least):
        _fail(name, f"{arg} must be a finite number{'' if least is None else f' >= {least}'}, got {x!r}")
    return y


def _vector(name: str, arg: str, t, dtype, n: Optional[int], device) -> torch.Tensor:
    t = _args.gpu_tensor(_fail, name, arg, t, dtype, device)
    if t.dim() != 1 or (n is not None and int(t.shape[0]) != n):
        _fail(name, f"{arg} must have shape [{'N' if n is None else n}], got {tuple(t.shape)}")
    return t.contiguous()


def _check_adjacency(name: str, adj, n_vertices: int, n_triangles: int, device) -> VertexAdjacency:
    if not isinstance(adj, VertexAdjacency):
        _fail(name, f"adjacency must be None or a VertexAdjacency of this mesh, got {type(adj).__name__}")
    return VertexAdjacency(_vector(name, "adjacency.offsets", adj.offsets, torch.int32, n_vertices + 1, device),
                           _vector(name, "adjacency.neighbours", adj.neighbours, torch.int32, None, device),
                           _vector(name, "adjacency.face_offsets", adj.face_offsets, torch.int32, n_vertices + 1, device),
                           _vector(name, "adjacency.faces_of", adj.faces_of, torch.int32, None, device),
                           _vector(name, "adjacency.irregular", adj.irregular, torch.uint8, n_vertices, device),
                           _vector(name, "adjacency.valid", adj.valid, torch.uint8, n_triangles, device))


def _empty_adjacency(n_vertices: int, n_triangles: int, device) -> VertexAdjacency:
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=device)      # noqa: E731
    return VertexAdjacency(z(n_vertices + 1, torch.int32), z(0, torch.int32), z(n_vertices + 1, torch.int32), z(0, torch.int32), z(n_vertices, torch.uint8),
                           z(n_triangles, torch.uint8))


def _adjacency(faces: torch.Tensor, n_vertices: int) -> VertexAdjacency:
    """Keys on the device, two ``torch.sort``, the rows kernel, then integer compaction in torch.  One readback: the two list lengths."""
    dev = faces.device
    Nt, Nv = int(faces.shape[0]), int(n_vertices)
    if Nt == 0 or Nv == 0:
        return _empty_adjacency(Nv, Nt, dev)
    lib, ctx, stream = _args.lib_and_stream(dev)
    valid = torch.empty(Nt, dtype=torch.uint8, device=dev)
    ekeys = torch.empty(6 * Nt, dtype=torch.int64, device=dev)
    fkeys = torch.empty(3 * Nt, dtype=torch.int64, device=dev)
    with ctx:
        _capi.check(lib.tsamd_smooth_keys(_ptr(faces), Nt, Nv, _ptr(valid), _ptr(ekeys), _ptr(fkeys), stream))
    ekeys = torch.sort(ekeys)[0]
    fkeys = torch.sort(fkeys)[0]                                          # unique but for the sentinels: a valid face names a vertex once
    head = torch.empty(6 * Nt, dtype=torch.uint8, device=dev)
    irregular = torch.empty(Nv, dtype=torch.uint8, device=dev)
    with ctx:
        _capi.check(lib.tsamd_smooth_rows(_ptr(ekeys), 6 * Nt, Nv, _ptr(head), _ptr(irregular), stream))
    n_rows, n_valid = (int(x) for x in torch.stack([head.sum(dtype=torch.int64), valid.sum(dtype=torch.int64)]).cpu().numpy())   # the one readback
    rows = ekeys[head != 0]
    assert int(rows.shape[0]) == n_rows
    live = fkeys[:3 * n_valid]
    at = torch.arange(Nv + 1, dtype=torch.int64, device=dev)
    offsets = torch.searchsorted(rows >> 32, at).to(torch.int32)          # integers: the first row whose source is >= i
    face_offsets = torch.searchsorted(live >> 32, at).to(torch.int32)
    return VertexAdjacency(offsets, (rows & 0xFFFFFFFF).to(torch.int32), face_offsets, (live & 0xFFFFFFFF).to(torch.int32), irregular, valid)


def _mesh_struct(adj: VertexAdjacency, faces: torch.Tensor, n_vertices: int) -> _capi.SmoothMeshStruct:
    m = _capi.SmoothMeshStruct()
    m.struct_size = ctypes.sizeof(_capi.SmoothMeshStruct)
    m.n_vertices, m.n_triangles = n_vertices, int(faces.shape[0])
    m.n_neighbours, m.n_face_entries = int(adj.neighbours.shape[0]), int(adj.faces_of.shape[0])
    m.offsets_dev, m.neighbours_dev = _ptr(adj.offsets), _ptr(adj.neighbours)
    m.face_offsets_dev, m.faces_of_dev, m.faces_dev = _ptr(adj.face_offsets), _ptr(adj.faces_of), _ptr(faces)
    return m


def _classify(v, mesh, adj, pinned, boundary):
    lib, ctx, stream = _args.lib_and_stream(v.device)
    cls = torch.empty(int(v.shape[0]), dtype=torch.uint8, device=v.device)
    with ctx:
        _capi.check(lib.tsamd_smooth_classify(_ptr(v), ctypes.byref(mesh), _ptr(adj.irregular), None if pinned is None else _ptr(pinned), BOUNDARIES[boundary],
                                              _ptr(cls), stream))
    return cls


def _run(v, mesh, cls, iterations, mode, lam, mu, max_move, stride=STATE_STRIDE):
    """The float64 state ``[Nv, 3]`` after ``iterations`` iterations (a view of the buffer that holds the result), enqueued."""
    Nv = int(v.shape[0])
    lib, ctx, stream = _args.lib_and_stream(v.device)
    a = torch.zeros((Nv, stride), dtype=torch.float64, device=v.device)
    a[:, :3] = v.double()
    b = torch.empty_like(a)                                              # every half-step writes all of its destination
    in_b = ctypes.c_int32()
    with ctx:
        _capi.check(lib.tsamd_smooth_run(_ptr(a), _ptr(b), stride, ctypes.byref(mesh), _ptr(cls), MODES[mode], lam, mu, iterations,
                                         None if max_move is None else _ptr(v), 0.0 if max_move is None else max_move, ctypes.byref(in_b), stream))
    return (b if in_b.value else a)[:, :3]


def _smooth(name, v, faces, iterations, mode, lam, mu, boundary, pinned, max_move, project, adj, stride=STATE_STRIDE):
    """``(out float32 [Nv, 3], counts)`` after the checks.  One readback: the four counts."""
    Nv = int(v.shape[0])
    mesh = _mesh_struct(adj, faces, Nv)
    cls = _classify(v, mesh, adj, pinned, boundary)
    counts = torch.bincount(cls.long(), minlength=4)
    state = _run(v, mesh, cls, iterations, mode, lam, mu, max_move, stride) if iterations else v.double()
    moves = (cls == 0)[:, None]
    out = torch.where(moves, state.float(), v)                           # a held vertex: its input bits
    if project:
        from . import metrics
        out = torch.where(moves, metrics._nearest_on_mesh(out.contiguous(), v, faces, 0, True)[2], v)
    return out.contiguous(), tuple(int(x) for x in counts.cpu().numpy()[:4])


# ---- the public interface ----
def adjacency(faces: torch.Tensor, n_vertices: int) -> VertexAdjacency:
    """The vertex adjacency of ``faces`` int32 ``[Nt, 3]`` over ``n_vertices`` vertices (:class:`VertexAdjacency`): directed edge keys from the
    device, ``torch.sort``, one pass over the runs, integer scans.  One readback.  Worth having on its own, and :func:`smooth` accepts
    it back, so that a frozen connectivity is analysed once."""
    name = "adjacency"
    faces = _args.typed_rows(_fail, name, "faces", faces, torch.int32, MAX_TRIANGLES)
    n_vertices = _args.integer(_fail, name, "n_vertices", n_vertices, 0, 2 ** 31 - 1, "2^31 - 1")
    return _adjacency(_args.placed(_fail, name, "faces", faces).contiguous(), n_vertices)      # what is wrong with an argument before where it is


def smooth(v: torch.Tensor, faces: torch.Tensor, iterations: int = 10, mode: str = DEFAULT_MODE, lam: float = 0.5, mu: float = -0.53, boundary: str = "fixed",
           pinned: Optional[torch.Tensor] = None, max_move: Optional[float] = None, project: bool = False,
           adjacency: Optional[VertexAdjacency] = None) -> SmoothedSurface:
    """Smooths the mesh ``v`` float32 ``[Nv, 3]``, ``faces`` int32 ``[Nt, 3]`` by ``iterations`` (0 .. 4096) iterations of ``mode`` (see the module
    text for both, for who moves and for what is not promised).  ``lam``, ``mu``: finite; a half-step whose coefficient is exactly 0 is
    skipped.  ``boundary``: ``"fixed"`` holds every vertex on an edge that is not in exactly two valid faces, ``"free"`` moves them too.
    ``pinned``: bool or uint8 ``[Nv]``, vertices to hold.  ``max_move=r`` (finite, >= 0): after every half-step each coordinate is clamped
    into ``[p0 - r, p0 + r]`` around the float64 input.  ``project=True``: after the last iteration every vertex that moved is replaced
    by :func:`tssplat_amd.metrics.nearest_on_mesh` of it on the INPUT mesh, which must then have a valid, finite triangle (one more
    readback finds out).  ``adjacency``: :func:`adjacency` of this mesh, to skip the analysis.  ``iterations=0`` returns a copy and the
    counts; an empty ``v`` or ``faces`` returns an unchanged copy without a device call.  A float64 state that overflows comes out as
    +-inf or NaN in float32.  One readback (two without ``adjacency``)."""
    name = "smooth"
    iterations = _args.integer(_fail, name, "iterations", iterations, 0, MAX_ITERATIONS)
    mode = _args.choice(_fail, name, "mode", mode, tuple(MODES))
    lam, mu = _number(name, "lam", lam), _number(name, "mu", mu)
    boundary = _args.choice(_fail, name, "boundary", boundary, tuple(BOUNDARIES))
    max_move = None if max_move is None else _number(name, "max_move", max_move, 0)
    if not isinstance(project, bool):
        _fail(name, f"project must be a bool, got {project!r}")
    v, faces_c = _check_mesh(name, v, faces)
    Nv, Nt = int(v.shape[0]), int(faces_c.shape[0])
    if pinned is not None:
        _args.on_gpu(_fail, name, "pinned", pinned)
        if pinned.dtype not in (torch.bool, torch.uint8):
            _fail(name, f"pinned must be bool or uint8, got {str(pinned.dtype).replace('torch.', '')}")
        pinned = _vector(name, "pinned", pinned, pinned.dtype, Nv, v.device).to(torch.uint8)
    if adjacency is not None:
        adjacency = _check_adjacency(name, adjacency, Nv, Nt, v.device)
    record = functools.partial(SmoothedSurface, faces=faces, iterations=iterations, mode=mode, lam=lam, mu=mu, boundary=boundary, max_move=max_move,
                               project=project)
    if Nv == 0 or Nt == 0:                                                # nothing has a neighbour
        if project:
            _fail(name, "project=True needs a valid triangle with finite corners to project onto; the input has none")
        return record(v=v.clone(), moved=0, held_other=Nv, held_pinned=0, held_irregular=0)
    adj = _adjacency(faces_c, Nv) if adjacency is None else adjacency
    if project:
        finite = torch.isfinite(v).all(1)
        f = faces_c.long().clamp(0, Nv - 1)
        if not bool(((adj.valid != 0) & finite[f[:, 0]] & finite[f[:, 1]] & finite[f[:, 2]]).any()):
            _fail(name, "project=True needs a valid triangle with finite corners to project onto; the input has none")
    out, (moved, other, held_pinned, irregular) = _smooth(name, v, faces_c, iterations, mode, lam, mu, boundary, pinned, max_move, project, adj)
    return record(v=out, moved=moved, held_other=other, held_pinned=held_pinned, held_irregular=irregular)
