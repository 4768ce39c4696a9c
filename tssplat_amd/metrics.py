"""Surface metrics on the device: area-uniform surface samples, nearest points, the exact point-to-triangle search, Chamfer distance,
F-score, normal consistency.

What the fit and the merge could not say so far is how good a surface is in 3-D.  This is the standard evaluation trio on
sampled surfaces: :func:`sample_surface` draws points uniformly in area, :func:`nearest` finds for every point of one set the
closest point of the other, and :func:`compare` turns the two directions into the figures of :class:`SurfaceMetrics`.  The
kernels sit behind ``tsamd_sample_surface`` and ``tsamd_nearest_points`` (include/tssplat_amd.h), stated in separately rounded
operations and integer minima so that they are bitwise repeatable; tests/metrics_oracle.py is the same statement in numpy and
Python integers.  There is no CPU fallback.

The search is brute force over all pairs, ``d2 = ((qx - rx)^2 + (qy - ry)^2) + (qz - rz)^2`` in float32 -- never the expanded form
``|q|^2 + |r|^2 - 2 q.r``, which cancels.  Sampled-against-sampled distances do not go to zero for identical surfaces:
:func:`compare_meshes` therefore returns a ``noise_floor`` with every record, the ``chamfer_l1`` of the reference sampled with two
different seeds.

:func:`nearest_on_mesh` is the distance from a point to a *mesh*: per query the closest triangle, the squared distance and the closest
point, by Ericson's Voronoi regions in float64 on the float32 inputs (``tsamd_nearest_on_mesh``; tests/pointmesh_oracle.py is the same
statement in numpy, and the device equals it bit for bit).  It is brute force over all pairs too, with a float32 bounding-sphere test
in front of the float64 evaluation that never changes the result.  :func:`compare_meshes_exact` measures samples against meshes with
it: a mesh against itself gives rounding-level figures, and its ``noise_floor`` says so.  The same search projects points onto a
surface or carries attributes from one mesh to another (``tri`` and ``point`` per query).

Out of scope: a cell grid or tree that prunes the search (the brute-force kernels are the specification any such search must
equal); signed distances; gradients of the distance and a Chamfer loss; mesh-quality figures.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools

import numpy as np
import torch

from . import _args, _capi

__all__ = ["SurfaceSamples", "SurfaceMetrics", "ThresholdMetrics", "NearestInfo", "NearestOnMeshInfo", "sample_surface", "nearest", "nearest_info",
           "nearest_on_mesh", "nearest_on_mesh_info", "compare", "compare_meshes", "compare_meshes_exact", "MAX_COUNT", "DEFAULT_THRESHOLDS"]

MAX_COUNT = 2 ** 31 - 1                 # triangles, samples, queries, ref points (include/tssplat_amd.h)
DEFAULT_THRESHOLDS = (0.01, 0.02)
_SAMPLE_WEIGHTS, _SAMPLE_DRAW = _capi.TSAMD_SAMPLE_WEIGHTS, _capi.TSAMD_SAMPLE_DRAW    # include/tssplat_amd.h


@dataclasses.dataclass
class SurfaceSamples:
    """``n`` points drawn uniformly in area, the unit normal of each point's triangle and that triangle's index."""
    points: torch.Tensor             # float32 [n, 3]
    normals: torch.Tensor            # float32 [n, 3]
    tri: torch.Tensor                # int32 [n]


@dataclasses.dataclass
class ThresholdMetrics:
    """At distance ``tau`` (the mesh's own units): ``precision = precision_count / N``, the share of ``a``'s samples within ``tau`` of
    ``b``; ``recall = recall_count / M`` the other way round; ``fscore`` their harmonic mean (0 when both are 0)."""
    tau: float
    precision: float
    recall: float
    fscore: float
    precision_count: int
    recall_count: int


@dataclasses.dataclass
class SurfaceMetrics:
    """``a`` is the surface under test, ``b`` the reference; ``d_ab`` the distance from a sample of ``a`` to the nearest sample of ``b``.
    ``chamfer_l1 = (mean d_ab + mean d_ba) / 2``; ``chamfer_l2 = mean d_ab^2 + mean d_ba^2``; ``accuracy = mean d_ab`` and
    ``completeness = mean d_ba`` with their maxima (one-sided Hausdorff estimates); ``normal_consistency`` the mean absolute cosine
    between a sample's normal and its nearest sample's, averaged over both directions.  Samples without a nearest point (every
    pair a NaN) are left out of the means and counted in ``dropped_ab`` / ``dropped_ba``.  ``noise_floor``: :func:`compare_meshes`."""
    n_a: int
    n_b: int
    chamfer_l1: float
    chamfer_l2: float
    accuracy: float
    completeness: float
    accuracy_max: float
    completeness_max: float
    normal_consistency: float
    dropped_ab: int
    dropped_ba: int
    thresholds: list
    noise_floor: float | None = None

    def as_dict(self) -> dict:
        return dataclasses.asdict(self)


@dataclasses.dataclass
class NearestInfo:
    """The compiled constants of the search kernel and the chunk count its automatic rule picks for ``n`` queries, ``m`` ref points."""
    block: int
    queries_per_lane: int
    ref_tile: int
    auto_chunks: int


@dataclasses.dataclass
class NearestOnMeshInfo:
    """The compiled constants of the point-to-triangle search and the chunk count its automatic rule picks for ``n`` queries, ``t`` triangles."""
    block: int
    queries_per_lane: int
    tri_tile: int
    auto_chunks: int


# ---- argument checks: the shared ones live in tssplat_amd/_args.py; here are the order and what only this module checks ----
_fail = functools.partial(_args.fail, "metrics")


def _check_n3(name: str, arg: str, t, dtype, device=None) -> torch.Tensor:
    """On a GPU, of ``dtype``, on ``device``, ``[N, 3]`` with at most MAX_COUNT rows; a tensor that is not contiguous is refused."""
    t = _args.gpu_tensor(_fail, name, arg, t, dtype, device)
    _args.rows(_fail, name, arg, t, 3, MAX_COUNT, "[N, 3] with N <= 2^31 - 1")
    if not t.is_contiguous():
        _fail(name, f"{arg} must be contiguous")
    return t


def _check_count(name: str, arg: str, n, least: int = 0) -> int:
    return _args.integer(_fail, name, arg, n, least, MAX_COUNT, "2^31 - 1")


def _check_seed(name: str, seed) -> int:
    if not _args.is_int(seed):
        _fail(name, f"seed must be an integer, got {seed!r}")
    return int(seed) & (2 ** 64 - 1)


def _check_thresholds(name: str, thresholds) -> tuple:
    try:
        taus = tuple(float(t) for t in thresholds)
    except (TypeError, ValueError):
        taus = (float("nan"),)
    if any(not (t >= 0.0 and np.isfinite(np.float32(t))) for t in taus):
        _fail(name, f"thresholds must be finite distances >= 0, got {thresholds!r}")
    return taus


def _check_samples(name: str, arg: str, s, device=None) -> SurfaceSamples:
    if not isinstance(s, SurfaceSamples):
        _fail(name, f"{arg} must be SurfaceSamples")
    points = _check_n3(name, f"{arg}.points", s.points, torch.float32, device)
    normals = _check_n3(name, f"{arg}.normals", s.normals, torch.float32, points.device)
    if normals.shape[0] != points.shape[0]:
        _fail(name, f"{arg}.normals must have {arg}.points' rows ({points.shape[0]}), got {normals.shape[0]}")
    if points.shape[0] == 0:
        _fail(name, f"{arg}.points holds no sample")
    return SurfaceSamples(points, normals, s.tri)


def nearest_info(n: int, m: int) -> NearestInfo:
    """Touches no device."""
    n, m = _check_count("nearest_info", "n", n), _check_count("nearest_info", "m", m)
    out = [C.c_int32() for _ in range(4)]
    _capi.check(_capi.load().tsamd_nearest_points_info(n, m, *(C.byref(x) for x in out)))
    return NearestInfo(*(int(x.value) for x in out))


def sample_surface(v: torch.Tensor, faces: torch.Tensor, n: int, seed: int = 0) -> SurfaceSamples:
    """``n`` independent samples of the triangle mesh ``v`` float32 ``[V, 3]``, ``faces`` int32 ``[T, 3]``, uniform in area.  A triangle with
    an index outside ``[0, V)``, a coordinate that is not finite or no area is never drawn.  The draws are counter-based: sample ``i`` of
    ``seed`` is the same whatever ``n`` is, on every run.  A surface without a triangle of positive area is an error.  One readback (the
    total weight)."""
    name = "sample_surface"
    v = _check_n3(name, "v", v, torch.float32)
    faces = _check_n3(name, "faces", faces, torch.int32, v.device)
    n = _check_count(name, "n", n)
    seed = _check_seed(name, seed)
    T = int(faces.shape[0])
    if T == 0:
        _fail(name, "faces holds no triangle")
    lib, ctx, stream = _args.lib_and_stream(v.device)
    dev = v.device
    q = torch.empty(T, dtype=torch.int64, device=dev)
    workspace = torch.empty(1, dtype=torch.int64, device=dev)
    with ctx:
        _capi.check(lib.tsamd_sample_surface(_SAMPLE_WEIGHTS, _args.ptr(v), int(v.shape[0]), faces.data_ptr(), T, q.data_ptr(), workspace.data_ptr(), 0, 0, None,
                                             None, None, stream))
    prefix = torch.cumsum(q, 0)                                     # integers: any scan order gives the same bits
    if int(prefix[-1].cpu()) <= 0:                                  # the one readback
        _fail(name, "faces holds no triangle of positive area with finite vertices: there is nothing to sample")
    out = SurfaceSamples(torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty((n, 3), dtype=torch.float32, device=dev),
                         torch.empty(n, dtype=torch.int32, device=dev))
    if n:
        with ctx:
            _capi.check(lib.tsamd_sample_surface(_SAMPLE_DRAW, _args.ptr(v), int(v.shape[0]), faces.data_ptr(), T, prefix.data_ptr(), None, n, seed,
                                                 out.points.data_ptr(), out.normals.data_ptr(), out.tri.data_ptr(), stream))
    return out


def _nearest(name, query, ref, ref_chunks):
    N, M = int(query.shape[0]), int(ref.shape[0])
    dev = query.device
    d2 = torch.empty(N, dtype=torch.float32, device=dev)
    idx = torch.empty(N, dtype=torch.int32, device=dev)
    if N == 0:
        return d2, idx
    lib, ctx, stream = _args.lib_and_stream(dev)
    workspace = torch.empty(int(lib.tsamd_nearest_points_workspace_bytes(N)) // 8, dtype=torch.int64, device=dev)
    with ctx:
        _capi.check(lib.tsamd_nearest_points(query.data_ptr(), N, ref.data_ptr(), M, ref_chunks, workspace.data_ptr(), d2.data_ptr(), idx.data_ptr(), stream))
    return d2, idx


def nearest(query: torch.Tensor, ref: torch.Tensor, ref_chunks: int = 0):
    """``(d2 float32 [N], idx int32 [N])``: per row of ``query`` float32 ``[N, 3]`` the smallest ``d2 = ((qx - rx)^2 + (qy - ry)^2) + (qz - rz)^2``
    (float32, in that order) over the rows of ``ref`` float32 ``[M, 3]`` and the row it belongs to.  The lower row wins a tie; a pair
    whose ``d2`` is NaN is skipped; ``+inf`` is an ordinary value; a query with no pair left gets ``(+inf, -1)``.  ``ref_chunks``: into how
    many parts the kernel splits ``ref`` (0: automatic, :func:`nearest_info`); the result does not depend on it.  Nothing synchronises."""
    name = "nearest"
    query = _check_n3(name, "query", query, torch.float32)
    ref = _check_n3(name, "ref", ref, torch.float32, query.device)
    M = int(ref.shape[0])
    if M == 0:
        _fail(name, "ref holds no point")
    if not _args.is_int(ref_chunks, 0, min(M, 65535)):
        _fail(name, f"ref_chunks must be 0 (automatic) or an integer in 1 .. min(M, 65535) = {min(M, 65535)}, got {ref_chunks!r}")
    return _nearest(name, query, ref, int(ref_chunks))


def _side(d2, idx, n_self, n_other, tau2):
    """:func:`_side_rows` with the other side's normals gathered by ``idx``."""
    return _side_rows(d2, idx, n_self, n_other.double()[idx.clamp(min=0).long()], tau2)


def _side_rows(d2, idx, n_self, b, tau2):
    """float64 [6 + len(tau2)] on the device: dropped, kept, sum d, max d, sum d2, sum |cos|, then the counts d2 <= tau^2.  ``b``: float64
    ``[N, 3]``, the normal each row is compared with (any finite or NaN row where ``idx < 0``)."""
    keep = idx >= 0
    d = torch.sqrt(d2).double()                                     # float32 roots, float64 from here on
    zero = torch.zeros((), dtype=torch.float64, device=d2.device)
    a = n_self.double()
    cos = ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]).abs()
    kept = keep.sum()
    rows = [(~keep).sum().double(), kept.double(), torch.where(keep, d, zero).sum(), torch.where(keep, d, zero - 1).max(),
            torch.where(keep, d2.double(), zero).sum(), torch.where(keep, cos, zero).sum()]
    rows += [(keep & (d2 <= t)).sum().double() for t in tau2]
    return torch.stack(rows)


def _record(ab, ba, N, M, taus) -> SurfaceMetrics:
    """The record from the two rows of :func:`_side`, read back."""
    nan = float("nan")

    def mean(row, k):
        return float(row[k] / row[1]) if row[1] > 0 else nan
    th = []
    for k, t in enumerate(taus):
        pc, rc = int(ab[6 + k]), int(ba[6 + k])
        P, R = pc / N, rc / M
        th.append(ThresholdMetrics(float(t), P, R, 2 * P * R / (P + R) if P + R > 0 else 0.0, pc, rc))
    return SurfaceMetrics(n_a=N, n_b=M, chamfer_l1=0.5 * (mean(ab, 2) + mean(ba, 2)), chamfer_l2=mean(ab, 4) + mean(ba, 4), accuracy=mean(ab, 2),
                          completeness=mean(ba, 2), accuracy_max=float(ab[3]) if ab[1] > 0 else nan, completeness_max=float(ba[3]) if ba[1] > 0 else nan,
                          normal_consistency=0.5 * (mean(ab, 5) + mean(ba, 5)), dropped_ab=int(ab[0]), dropped_ba=int(ba[0]), thresholds=th)


def _compare(name, a: SurfaceSamples, b: SurfaceSamples, taus) -> SurfaceMetrics:
    d2_ab, idx_ab = _nearest(name, a.points, b.points, 0)
    d2_ba, idx_ba = _nearest(name, b.points, a.points, 0)
    tau2 = [float(np.float32(t) * np.float32(t)) for t in taus]     # fl32(tau)^2 in float32, compared with the float32 d2
    # plain torch reductions in float64 (no atomics: the same tensors give the same bits), one readback for the whole record
    ab, ba = torch.stack([_side(d2_ab, idx_ab, a.normals, b.normals, tau2), _side(d2_ba, idx_ba, b.normals, a.normals, tau2)]).cpu().numpy()
    return _record(ab, ba, int(a.points.shape[0]), int(b.points.shape[0]), taus)


def compare(a: SurfaceSamples, b: SurfaceSamples, thresholds=DEFAULT_THRESHOLDS) -> SurfaceMetrics:
    """The figures of :class:`SurfaceMetrics` from two :func:`nearest` calls, ``a`` -> ``b`` and ``b`` -> ``a``.  ``a`` is the surface under test,
    ``b`` the reference.  The same samples give the same record, bit for bit.  One readback."""
    name = "compare"
    a = _check_samples(name, "a", a)
    b = _check_samples(name, "b", b, a.points.device)
    return _compare(name, a, b, _check_thresholds(name, thresholds))


def compare_meshes(v_a, f_a, v_b, f_b, n: int = 100_000, seed: int = 0, thresholds=DEFAULT_THRESHOLDS) -> SurfaceMetrics:
    """:func:`compare` of ``n`` samples of mesh ``a`` (the surface under test, drawn with ``seed + 2``) and ``n`` samples of mesh ``b`` (the
    reference, drawn with ``seed``).  ``noise_floor``: the ``chamfer_l1`` of ``b`` sampled with ``seed`` against ``b`` sampled with ``seed + 1`` --
    what two samplings of one surface are apart at this density; a ``chamfer_l1`` near it says "the same surface as far as ``n`` samples
    can tell".  The three streams are independent, so a mesh against itself gives about its floor, not 0."""
    name = "compare_meshes"
    n = _check_count(name, "n", n, least=1)
    seed = _check_seed(name, seed)
    taus = _check_thresholds(name, thresholds)
    v_a = _check_n3(name, "v_a", v_a, torch.float32)
    f_a = _check_n3(name, "f_a", f_a, torch.int32, v_a.device)
    v_b = _check_n3(name, "v_b", v_b, torch.float32, v_a.device)
    f_b = _check_n3(name, "f_b", f_b, torch.int32, v_a.device)
    a = sample_surface(v_a, f_a, n, seed + 2)
    b = sample_surface(v_b, f_b, n, seed)
    b2 = sample_surface(v_b, f_b, n, seed + 1)
    rec = _compare(name, a, b, taus)
    rec.noise_floor = _compare(name, b, b2, taus).chamfer_l1
    return rec


# ---- the exact point-to-triangle search ----
def nearest_on_mesh_info(n: int, t: int) -> NearestOnMeshInfo:
    """Touches no device."""
    n, t = _check_count("nearest_on_mesh_info", "n", n), _check_count("nearest_on_mesh_info", "t", t)
    out = [C.c_int32() for _ in range(4)]
    _capi.check(_capi.load().tsamd_nearest_on_mesh_info(n, t, *(C.byref(x) for x in out)))
    return NearestOnMeshInfo(*(int(x.value) for x in out))


def _nearest_on_mesh(query, v, faces, ref_chunks, return_points):
    N, T = int(query.shape[0]), int(faces.shape[0])
    dev = query.device
    d2 = torch.empty(N, dtype=torch.float32, device=dev)
    tri = torch.empty(N, dtype=torch.int32, device=dev)
    point = torch.empty((N, 3), dtype=torch.float32, device=dev) if return_points else None
    if N == 0:
        return d2, tri, point
    lib, ctx, stream = _args.lib_and_stream(dev)
    workspace = torch.empty((int(lib.tsamd_nearest_on_mesh_workspace_bytes(N, T)) + 15) // 16 * 2, dtype=torch.int64, device=dev)
    with ctx:
        _capi.check(lib.tsamd_nearest_on_mesh(query.data_ptr(), N, _args.ptr(v), int(v.shape[0]), faces.data_ptr(), T, ref_chunks, workspace.data_ptr(),
                                              d2.data_ptr(), tri.data_ptr(), point.data_ptr() if return_points else None, stream))
    return d2, tri, point


def nearest_on_mesh(query: torch.Tensor, v: torch.Tensor, faces: torch.Tensor, ref_chunks: int = 0, return_points: bool = True):
    """``(d2 float32 [N], tri int32 [N], point float32 [N, 3] or None)``: per row of ``query`` float32 ``[N, 3]`` the closest triangle of the mesh
    ``v`` float32 ``[V, 3]``, ``faces`` int32 ``[T, 3]``, the squared distance to it and the closest point on it -- the float64 statement of
    tests/pointmesh_oracle.py and include/tssplat_amd.h, each rounded once to float32.  A triangle with an index outside ``[0, V)``, a
    coordinate that is not finite or no area is never a result; the lowest triangle wins a tie; a pair whose ``d2`` is NaN is skipped; a
    query with no pair left gets ``(+inf, -1)`` and a NaN point, so a mesh without a valid triangle is not an error.  ``ref_chunks``: into
    how many parts the kernel splits the triangles (0: automatic, :func:`nearest_on_mesh_info`); the result does not depend on it.
    Nothing synchronises."""
    name = "nearest_on_mesh"
    query = _check_n3(name, "query", query, torch.float32)
    v = _check_n3(name, "v", v, torch.float32, query.device)
    faces = _check_n3(name, "faces", faces, torch.int32, query.device)
    T = int(faces.shape[0])
    if T == 0:
        _fail(name, "faces holds no triangle")
    if not _args.is_int(ref_chunks, 0, min(T, 65535)):
        _fail(name, f"ref_chunks must be 0 (automatic) or an integer in 1 .. min(T, 65535) = {min(T, 65535)}, got {ref_chunks!r}")
    if not isinstance(return_points, bool):
        _fail(name, f"return_points must be a bool, got {return_points!r}")
    return _nearest_on_mesh(query, v, faces, int(ref_chunks), return_points)


def _winning_normals(v, faces, tri):
    """float64 ``[N, 3]`` on the device: the unit normal ``(b - a) x (c - a) / w`` of triangle ``tri`` per row, in float64 torch on the gathered
    rows, each component two products and a difference as the sampler states them.  Rows with ``tri < 0`` are not used."""
    if int(v.shape[0]) == 0:
        return torch.full((int(tri.shape[0]), 3), float("nan"), dtype=torch.float64, device=tri.device)
    f = faces[tri.clamp(min=0).long()].long().clamp(0, int(v.shape[0]) - 1)          # a winning triangle's indices are in range as they are
    a, b, c = (v[f[:, k]].double() for k in range(3))
    e1, e2 = b - a, c - a
    n = torch.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], dim=1)
    return n / torch.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])[:, None]


def compare_meshes_exact(v_a, f_a, v_b, f_b, n: int = 100_000, seed: int = 0, thresholds=DEFAULT_THRESHOLDS) -> SurfaceMetrics:
    """:func:`compare_meshes` with exact distances: ``n`` samples of mesh ``a`` (drawn with ``seed + 2``) are searched against the triangles
    of mesh ``b`` and ``n`` samples of ``b`` (``seed``) against the triangles of ``a`` (:func:`nearest_on_mesh`); ``d = sqrt(d2)`` and the same
    float64 reductions give the same fields, with the normal consistency taken against the unit normal of the winning triangle.
    ``noise_floor``: the ``accuracy`` of ``b`` sampled with ``seed + 1`` against mesh ``b`` itself -- the samples lie on the mesh, so this is
    the rounding of the sampler and the search (about 1e-8 of the mesh's size), reported so that the reader sees that the figures have
    no sampling floor.  One readback."""
    name = "compare_meshes_exact"
    n = _check_count(name, "n", n, least=1)
    seed = _check_seed(name, seed)
    taus = _check_thresholds(name, thresholds)
    v_a = _check_n3(name, "v_a", v_a, torch.float32)
    f_a = _check_n3(name, "f_a", f_a, torch.int32, v_a.device)
    v_b = _check_n3(name, "v_b", v_b, torch.float32, v_a.device)
    f_b = _check_n3(name, "f_b", f_b, torch.int32, v_a.device)
    a = sample_surface(v_a, f_a, n, seed + 2)
    b = sample_surface(v_b, f_b, n, seed)
    b2 = sample_surface(v_b, f_b, n, seed + 1)
    d2_ab, tri_ab, _ = _nearest_on_mesh(a.points, v_b, f_b, 0, False)
    d2_ba, tri_ba, _ = _nearest_on_mesh(b.points, v_a, f_a, 0, False)
    d2_fl, tri_fl, _ = _nearest_on_mesh(b2.points, v_b, f_b, 0, False)
    tau2 = [float(np.float32(t) * np.float32(t)) for t in taus]
    rows = torch.stack([_side_rows(d2_ab, tri_ab, a.normals, _winning_normals(v_b, f_b, tri_ab), tau2),
                        _side_rows(d2_ba, tri_ba, b.normals, _winning_normals(v_a, f_a, tri_ba), tau2),
                        _side_rows(d2_fl, tri_fl, b2.normals, _winning_normals(v_b, f_b, tri_fl), tau2)]).cpu().numpy()      # the one readback
    rec = _record(rows[0], rows[1], n, n, taus)
    rec.noise_floor = float(rows[2][2] / rows[2][1]) if rows[2][1] > 0 else float("nan")
    return rec
