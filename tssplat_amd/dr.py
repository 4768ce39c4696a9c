"""The nvdiffrast operators the reference's renderer uses, on the MI355X kernels.

/root/reference/renderers/mesh_rasterizer.py does ``import nvdiffrast.torch as dr`` (:2) and calls

    self.glctx = dr.RasterizeCudaContext()                                                          :34
    rast_out, _ = dr.rasterize(self.glctx, pos_clip, t_pos_idx, resolution=res, grad_db=False)      :103
    positions_all, _ = dr.interpolate(v_pos[None, ...], rast_out, t_pos_idx)                        :117  (:145, :153)
    alpha = dr.antialias(alpha, rast_out, pos_clip, t_pos_idx, topology_hash=None, pos_gradient_boost=1.0)   :107, :128

This module offers all four under the same names and argument order (``import tssplat_amd.dr as dr``), differentiable
where nvdiffrast is: ``rasterize`` w.r.t. ``pos`` through ``(u, v)``, ``interpolate`` w.r.t. ``attr`` and ``rast``,
``antialias`` w.r.t. ``color`` and ``pos``.  ``texture`` (which the reference's renderer does not call, but a textured mesh
exported by ``MeshRasterizer.export`` needs to be rendered again) is offered without mipmaps and cube maps, differentiable
w.r.t. ``tex`` and ``uv``; its semantics are pinned down in tests/texture_oracle.py, PARITY UNPINNED likewise.  nvdiffrast is a separate library, not vendored by the reference and not
installed here: the semantics are a restatement of its published algorithm, pinned down in oracle/raster_oracle.py --
PARITY UNPINNED against the library itself.

What it does not do, loudly: ``grad_db=True``, ``ranges`` (range mode) and ``rast_db`` / ``diff_attrs`` are
rejected (``RasterizeGLContext`` is an alias of the HIP context); clipping is against the NEAR plane only (a triangle with vertices at ``w <= 0`` is clipped there; one with a vertex
beyond the +-16384-pixel guard band is dropped; the silhouette of a clipped triangle is not antialiased); no depth peeling; ``texture`` rejects ``uv_da``,
``mip_level_bias``, ``mip``, ``max_mip_level``, the ``linear-mipmap-*`` filters and ``boundary_mode='cube'``.

``silhouette`` and ``silhouette_mse`` are this package's own: the alpha stage of the reference's trainer (``only_alpha=True``:
``MSE(antialias(clamp(rast[..., -1:], 0, 1)))``) without the ``rast`` image, the clamp, the antialias copy and the dense loss
gradient -- the same blends as the three operators above give on the 0 / 1 coverage image.  ``silhouette_depth_mse`` adds the
trainer's depth term (``fit_depth``: ``MSE(||interpolate(v_pos, rast) - campos|| * mask, target * mask)``) to that one rasterisation,
from the triangle ids the alpha stage leaves: no ``rast`` image, no interpolated image, no gradient image.  ``silhouette_normal_mse``
adds the normal term (``fit_normal``: a masked ``MSE`` of ``interpolate(vertex normals, rast)``) in the same way, with the depth term
beside it when asked: alpha, depth and normal from one rasterisation and one autograd node.

``plan_blends``, ``shade`` and ``shade_l1`` are this package's own too: the colour stage under frozen geometry and fixed views.
There the blends of ``antialias`` do not depend on what is being trained, so they are extracted once into a :class:`BlendPlan`,
and ``L1(antialias(lerp(background, scatter(color), mask)))`` becomes a fixed sparse operator on the ``[N, 3]`` point colours:
no image-sized temporary in either direction (``shade_l1`` writes an image only when asked to return it), no atomics, bitwise repeatable.
"""
from __future__ import annotations

import collections
import weakref

import os

import torch

from . import _capi
from .tet_spheres_ext import _device_ctx, _stream_ptr

__all__ = ["RasterizeCudaContext", "rasterize", "interpolate", "antialias", "antialias_construct_topology_hash", "texture", "silhouette",
           "silhouette_mse", "silhouette_depth_mse", "silhouette_normal_mse", "BlendPlan", "plan_blends", "shade", "shade_l1"]

_lib = _capi.load()


class RasterizeCudaContext:
    """``dr.RasterizeCudaContext()`` (mesh_rasterizer.py:34): holds the workspace (depth keys, snapped vertices) between calls."""

    def __init__(self, device=None):
        self.device = None if device is None else torch.device(device)
        self._ws = None

    def workspace(self, batch: int, n_vertices: int, height: int, width: int, device: torch.device) -> torch.Tensor:
        need = int(_lib.tsamd_rasterize_workspace_bytes(batch, n_vertices, height, width))
        if self._ws is None or self._ws.numel() < need or self._ws.device != device:
            self._ws = torch.empty(max(need, 8), dtype=torch.uint8, device=device)
        return self._ws


class RasterizeGLContext(RasterizeCudaContext):
    """``dr.RasterizeGLContext()`` (mesh_rasterizer.py:35-36, ``context_type == "gl"``).  nvdiffrast's second back end runs the same
    operators through OpenGL; there is no OpenGL on this platform and nothing in the operators' contract depends on it, so the
    name is served by the same HIP kernels (``output_db`` / ``mode`` are accepted and ignored: image-space derivatives are not
    offered by either context here)."""

    def __init__(self, output_db: bool = True, mode: str = "automatic", device=None):
        super().__init__(device)


def _check_cuda_f32(name: str, t: torch.Tensor) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"tssplat_amd.dr: {name} must be a GPU tensor (there is no CPU fallback)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"tssplat_amd.dr: {name} must be float32")
    return t.contiguous()


def _ptr(t):
    """The address of ``t`` for the C ABI; ``None`` (a null pointer) for ``None`` or an empty tensor."""
    return t.data_ptr() if t is not None and t.numel() else None


# TSSPLAT_AMD_DR_CHECK=1: count, on every rasterize call, the triangles this slice DROPS -- a vertex that is not finite or
# outside the +-16384-pixel guard band (a finite vertex at w <= 0 is clipped against the near plane, not dropped) -- and warn.
# A device read per call: a debugging aid, off by default (objects inside the frustum, the reference's case, lose nothing).
_CHECK_DROPPED = os.environ.get("TSSPLAT_AMD_DR_CHECK", "0") == "1"


def count_dropped_triangles(pos: torch.Tensor, tri: torch.Tensor, height: int, width: int) -> int:
    """(view, triangle) pairs that ``rasterize`` drops whole (see the module docstring)."""
    with torch.no_grad():
        w = pos[..., 3]
        finite = torch.isfinite(pos).all(dim=-1)
        front = finite & (w > 0)
        ws = torch.where(front, w, torch.ones_like(w))
        sx = (pos[..., 0] / ws * 0.5 + 0.5) * width
        sy = (pos[..., 1] / ws * 0.5 + 0.5) * height
        ok = (front & (sx.abs() <= 16384.0) & (sy.abs() <= 16384.0)) | (finite & (w <= 0))    # (w <= 0: clipped at the near plane)
        t = tri.long()
        bad = ~(ok[:, t[:, 0]] & ok[:, t[:, 1]] & ok[:, t[:, 2]])
        return int(bad.sum())


def _warn_dropped(pos, tri, height, width) -> None:
    n = count_dropped_triangles(pos, tri, height, width)
    if n:
        import warnings
        warnings.warn(f"tssplat_amd.dr.rasterize: {n} (view, triangle) pairs have a vertex that is not finite or beyond the +-16384-pixel "
                      f"guard band and are DROPPED whole", RuntimeWarning, stacklevel=3)


def _check_pos(name: str, pos: torch.Tensor, batch=None) -> torch.Tensor:
    pos = _check_cuda_f32("pos", pos)
    if pos.dim() != 3 or pos.shape[2] != 4 or (batch is not None and pos.shape[0] != batch):
        raise RuntimeError(f"tssplat_amd.dr.{name}: pos must be [B, V, 4] clip-space positions (instanced mode)")
    return pos


def _check_resolution(name: str, resolution, n_triangles: int):
    """``(height, width)`` within the limits of this slice (include/tssplat_amd.h): the triangle id + 1 travels as a float32 (exact
    up to 2^24), and window coordinates are snapped within +-16384 pixels -- a triangle with a vertex beyond that guard band is
    dropped whole (one with vertices at w <= 0 is clipped against the near plane): harmless for objects inside the frustum, which
    the reference renders."""
    height, width = int(resolution[0]), int(resolution[1])
    if n_triangles > (1 << 24) - 1:
        raise RuntimeError(f"tssplat_amd.dr.{name}: more than 2^24 - 1 triangles")
    if not (0 <= height <= 8192 and 0 <= width <= 8192):
        raise RuntimeError(f"tssplat_amd.dr.{name}: resolution out of range (0 .. 8192 pixels per side)")
    return height, width


def _check_tri(tri: torch.Tensor, device) -> torch.Tensor:
    if not isinstance(tri, torch.Tensor) or tri.dim() != 2 or tri.shape[1] != 3:
        raise RuntimeError("tssplat_amd.dr: tri must be an [T, 3] tensor")
    if tri.dtype != torch.int32:
        raise RuntimeError("tssplat_amd.dr: tri must be int32 (as nvdiffrast requires)")
    if tri.device != device:
        raise RuntimeError("tssplat_amd.dr: tri must live on the same device as pos / rast")
    return tri.contiguous()


class _RasterizeFunc(torch.autograd.Function):
    """``rast`` with the gradient of its ``(u, v)`` channels w.r.t. ``pos`` (tsamd_rasterize_backward)."""

    @staticmethod
    def forward(ctx, pos, tri, glctx, height, width, pair_masks):
        B, V = int(pos.shape[0]), int(pos.shape[1])
        rast = torch.empty((B, height, width, 4), dtype=torch.float32, device=pos.device)
        ws = glctx.workspace(B, V, height, width, pos.device)
        with _device_ctx(pos.device):
            _capi.check(_lib.tsamd_rasterize(pos.data_ptr(), B, V, tri.data_ptr(), int(tri.shape[0]), height, width, ws.data_ptr(),
                                             rast.data_ptr(), _ptr(pair_masks), _stream_ptr(pos.device)))
        ctx.save_for_backward(pos, tri, rast)
        return rast

    @staticmethod
    def backward(ctx, grad_rast):
        pos, tri, rast = ctx.saved_tensors
        B, V, H, W = int(pos.shape[0]), int(pos.shape[1]), int(rast.shape[1]), int(rast.shape[2])
        g = grad_rast.contiguous()
        grad_pos = torch.empty_like(pos)
        with _device_ctx(pos.device):
            _capi.check(_lib.tsamd_rasterize_backward(pos.data_ptr(), B, V, tri.data_ptr(), int(tri.shape[0]), H, W, rast.data_ptr(),
                                                      g.data_ptr(), grad_pos.data_ptr(), _stream_ptr(pos.device)))
        return grad_pos, None, None, None, None, None


# The pair masks of the last rasterised image per device (a by-product of the resolve pass, 2 bits per pixel: which pixels show a
# different triangle than their right / upper neighbour), for the antialias call that receives the SAME rast tensor unmodified --
# identity through a weak reference plus the version counter, as for the topology table below.  mesh_rasterizer.py:103-107 is
# exactly that sequence; any other use (a copy, a slice, an edited image) finds no masks and antialias scans the image itself.
# The by-product costs the resolve pass a second stream of depth keys (+0.06 ms at 120 views x 512^2), so it is produced only
# while it is being used: a rasterize call that finds the previous masks unclaimed stops producing them, an antialias call that
# finds none asks for them again.
PAIR_MASKS_FROM_RASTERIZE = os.environ.get("TSSPLAT_AMD_DR_PAIR_MASKS", "1") != "0"
_last_pair_masks: dict = {}     # device -> (masks, weakref(rast), version)
_pair_masks_wanted: dict = {}   # device -> bool (absent: yes)


def _pair_masks_for(rast: torch.Tensor):
    hit = _last_pair_masks.get(rast.device)
    if hit is not None:
        masks, ref, version = hit
        if ref() is rast and version == rast._version:
            del _last_pair_masks[rast.device]          # claimed
            return masks
    _pair_masks_wanted[rast.device] = True             # an antialias call without masks: the next rasterize makes them
    return None


def rasterize(glctx: RasterizeCudaContext, pos: torch.Tensor, tri: torch.Tensor, resolution, ranges=None, grad_db: bool = True):
    """``(rast, rast_db)``: ``rast[B, H, W, 4] = (u, v, z/w, triangle_id + 1)``, zeros on background; ``rast_db`` is an empty
    tensor (image-space derivatives are only produced with ``grad_db=True``, which is rejected: the reference passes False)."""
    if ranges is not None:
        raise NotImplementedError("tssplat_amd.dr.rasterize: range mode is not supported")
    if grad_db:
        raise NotImplementedError("tssplat_amd.dr.rasterize: grad_db=True is not supported (the reference passes grad_db=False)")
    pos = _check_pos("rasterize", pos)
    tri = _check_tri(tri, pos.device)
    height, width = _check_resolution("rasterize", resolution, int(tri.shape[0]))
    if _CHECK_DROPPED and tri.shape[0] > 0:
        _warn_dropped(pos, tri, height, width)
    masks = None
    if _last_pair_masks.pop(pos.device, None) is not None:
        _pair_masks_wanted[pos.device] = False         # the last ones were never claimed by an antialias call
    if PAIR_MASKS_FROM_RASTERIZE and _pair_masks_wanted.get(pos.device, True) and height * width > 0:
        masks = torch.empty((int(_lib.tsamd_pair_masks_bytes(int(pos.shape[0]), height, width)),), dtype=torch.uint8, device=pos.device)
    rast = _RasterizeFunc.apply(pos, tri, glctx, height, width, masks)
    if masks is not None:
        _last_pair_masks[pos.device] = (masks, weakref.ref(rast), rast._version)
    return rast, torch.empty((int(pos.shape[0]), height, width, 0), dtype=torch.float32, device=pos.device)


class _InterpolateFunc(torch.autograd.Function):
    @staticmethod
    def forward(ctx, attr, rast, tri):
        B, H, W = int(rast.shape[0]), int(rast.shape[1]), int(rast.shape[2])
        A, V, Cn = int(attr.shape[0]), int(attr.shape[1]), int(attr.shape[2])
        out = torch.empty((B, H, W, Cn), dtype=torch.float32, device=rast.device)
        with _device_ctx(rast.device):
            _capi.check(_lib.tsamd_interpolate(attr.data_ptr(), A, V, Cn, rast.data_ptr(), tri.data_ptr(), int(tri.shape[0]), B, H, W, out.data_ptr(),
                                               _stream_ptr(rast.device)))
        ctx.save_for_backward(attr, rast, tri)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        attr, rast, tri = ctx.saved_tensors
        B, H, W = int(rast.shape[0]), int(rast.shape[1]), int(rast.shape[2])
        A, V, Cn = int(attr.shape[0]), int(attr.shape[1]), int(attr.shape[2])
        g = grad_out.contiguous()
        grad_attr = torch.empty_like(attr)
        grad_rast = torch.empty_like(rast) if ctx.needs_input_grad[1] else None
        with _device_ctx(rast.device):
            _capi.check(_lib.tsamd_interpolate_backward(attr.data_ptr(), A, V, Cn, rast.data_ptr(), tri.data_ptr(), int(tri.shape[0]), B, H, W, g.data_ptr(),
                                                        grad_attr.data_ptr(), _ptr(grad_rast), _stream_ptr(rast.device)))
        return grad_attr, grad_rast, None


def interpolate(attr: torch.Tensor, rast: torch.Tensor, tri: torch.Tensor, rast_db=None, diff_attrs=None):
    """``(out, out_da)``: ``out[B, H, W, C] = u a0 + v a1 + (1 - u - v) a2``, 0 on background; ``out_da`` is an empty tensor
    (attribute derivatives need ``rast_db``, not part of this slice)."""
    if rast_db is not None or diff_attrs is not None:
        raise NotImplementedError("tssplat_amd.dr.interpolate: rast_db / diff_attrs are not part of this slice")
    rast = _check_cuda_f32("rast", rast)
    attr = _check_cuda_f32("attr", attr)
    if rast.dim() != 4 or rast.shape[3] != 4:
        raise RuntimeError("tssplat_amd.dr.interpolate: rast must be [B, H, W, 4]")
    if attr.dim() != 3 or attr.shape[0] not in (1, rast.shape[0]):
        raise RuntimeError("tssplat_amd.dr.interpolate: attr must be [1 or B, V, C]")
    if attr.device != rast.device:
        raise RuntimeError("tssplat_amd.dr.interpolate: attr and rast must live on the same device")
    tri = _check_tri(tri, rast.device)
    out = _InterpolateFunc.apply(attr, rast, tri)
    return out, torch.empty(tuple(rast.shape[:3]) + (0,), dtype=torch.float32, device=rast.device)


class TopologyHash:
    """``dr.antialias_construct_topology_hash(tri)``: the edge partner table of one triangle list (``opp[3 t + e]`` = the
    vertex across edge ``e`` of triangle ``t``, -1 on a boundary)."""

    def __init__(self, tri: torch.Tensor):
        tri = _check_tri(tri, tri.device)
        if not tri.is_cuda:
            raise RuntimeError("tssplat_amd.dr: tri must be a GPU tensor (there is no CPU fallback)")
        T = int(tri.shape[0])
        self.n_triangles = T
        self.opp = torch.empty(3 * T, dtype=torch.int32, device=tri.device)
        need = int(_lib.tsamd_antialias_topology_workspace_bytes(T))
        if need < 0:
            raise RuntimeError("tssplat_amd.dr: too many triangles for the topology table")
        ws = torch.empty(max(need, 8), dtype=torch.uint8, device=tri.device)
        with _device_ctx(tri.device):
            _capi.check(_lib.tsamd_antialias_topology(tri.data_ptr(), T, ws.data_ptr(), self.opp.data_ptr(), _stream_ptr(tri.device)))


def antialias_construct_topology_hash(tri: torch.Tensor) -> TopologyHash:
    return TopologyHash(tri)


_last_topology: dict = {}


def _topology_for(tri: torch.Tensor) -> TopologyHash:
    """``topology_hash=None``: nvdiffrast rebuilds the table on every call; the last one per device is kept here for as long as
    the SAME (alive, unmodified) index tensor comes back -- identity through a weak reference plus the version counter, not
    the address: a freed tensor whose storage a new one reuses can never be served the old table."""
    hit = _last_topology.get(tri.device)
    if hit is not None:
        topo, ref, version = hit
        if ref() is tri and version == tri._version:
            return topo
    topo = TopologyHash(tri)
    _last_topology[tri.device] = (topo, weakref.ref(tri), tri._version)
    return topo


def _mesh_args(name: str, pos, tri, topology_hash, device=None):
    """``(pos, tri, topo)`` of an operator that analyses silhouette edges: ``pos[B, V, 4]``, ``tri[T, 3]`` on ``device`` (default:
    where ``pos`` lives) and the edge partner table -- ``topology_hash``, or the kept one of this triangle list."""
    pos = _check_pos(name, pos)
    device = pos.device if device is None else device
    tri = _check_tri(tri, device)
    topo = _topology_for(tri) if topology_hash is None else topology_hash
    if not isinstance(topo, TopologyHash) or topo.n_triangles != int(tri.shape[0]) or topo.opp.device != device:
        raise RuntimeError(f"tssplat_amd.dr.{name}: topology_hash does not belong to this triangle list")
    return pos, tri, topo


# None: decide per call (see _AntialiasFunc.forward); True / False force the prepared / the per-pair form of the antialias analysis
PREPARE_ANTIALIAS = None


class _AntialiasFunc(torch.autograd.Function):
    @staticmethod
    def forward(ctx, color, rast, pos, tri, opp, boost, pair_masks):
        B, H, W, Cn = (int(k) for k in color.shape)
        V, T = int(pos.shape[1]), int(tri.shape[0])
        out = torch.empty_like(color)
        # window coordinates per (view, vertex), mask of the pixel pairs on two triangles, edge flags per (view, triangle): once
        # for the forward and the backward analysis -- when the mesh is small against the image (the reference's use: one object,
        # 120 views x 512^2).  With more triangles than pixels the per-vertex / per-triangle tables cost more than they save
        # (512 spheres in 8 views: 0.32 against 0.16 ms) and the kernels work everything out per pixel pair.
        prepare = PREPARE_ANTIALIAS if PREPARE_ANTIALIAS is not None else 4 * (V + T) <= H * W
        win = torch.empty((int(_lib.tsamd_antialias_prepared_bytes(B, V, T, H, W)) if prepare else 0,), dtype=torch.uint8, device=color.device)
        with _device_ctx(color.device):
            stream = _stream_ptr(color.device)
            if prepare:
                _capi.check(_lib.tsamd_antialias_prepare(rast.data_ptr(), pos.data_ptr(), tri.data_ptr(), opp.data_ptr(), _ptr(pair_masks), B, V, T, H, W,
                                                         win.data_ptr(), stream))
            _capi.check(_lib.tsamd_antialias(color.data_ptr(), rast.data_ptr(), pos.data_ptr(), win.data_ptr() if prepare else None, tri.data_ptr(),
                                             opp.data_ptr(), B, V, T, H, W, Cn, out.data_ptr(), stream))
        ctx.save_for_backward(color, rast, pos, tri, opp, win)
        ctx.boost = float(boost)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        color, rast, pos, tri, opp, win = ctx.saved_tensors
        B, H, W, Cn = (int(k) for k in color.shape)
        V, T = int(pos.shape[1]), int(tri.shape[0])
        g = grad_out.contiguous()
        grad_color = torch.empty_like(color) if ctx.needs_input_grad[0] else None
        grad_pos = torch.empty_like(pos) if ctx.needs_input_grad[2] else None
        if grad_color is None and grad_pos is None:
            return None, None, None, None, None, None, None
        with _device_ctx(color.device):
            _capi.check(_lib.tsamd_antialias_backward(color.data_ptr(), rast.data_ptr(), pos.data_ptr(), _ptr(win), tri.data_ptr(), opp.data_ptr(),
                                                      B, V, T, H, W, Cn, g.data_ptr(), ctx.boost, _ptr(grad_color), _ptr(grad_pos), _stream_ptr(color.device)))
        return grad_color, None, grad_pos, None, None, None, None


def antialias(color: torch.Tensor, rast: torch.Tensor, pos: torch.Tensor, tri: torch.Tensor, topology_hash=None, pos_gradient_boost: float = 1.0):
    """``dr.antialias`` (mesh_rasterizer.py:107,128): ``color[B, H, W, C]`` with the silhouette pixels blended by the position
    of the silhouette edge between the pixel centres; differentiable w.r.t. ``color`` and ``pos`` (``rast`` carries none)."""
    color = _check_cuda_f32("color", color)
    pair_masks = _pair_masks_for(rast)              # (by identity of the tensor dr.rasterize handed out)
    rast = _check_cuda_f32("rast", rast.detach())
    pos = _check_cuda_f32("pos", pos)
    if color.dim() != 4 or rast.dim() != 4 or rast.shape[3] != 4 or tuple(color.shape[:3]) != tuple(rast.shape[:3]):
        raise RuntimeError("tssplat_amd.dr.antialias: color must be [B, H, W, C] and rast [B, H, W, 4] of the same image size")
    pos = _check_pos("antialias", pos, rast.shape[0])
    if color.device != rast.device or pos.device != rast.device:
        raise RuntimeError("tssplat_amd.dr.antialias: color, rast and pos must live on the same device")
    pos, tri, topo = _mesh_args("antialias", pos, tri, topology_hash, rast.device)
    return _AntialiasFunc.apply(color, rast, pos, tri, topo.opp, float(pos_gradient_boost), pair_masks)


# ---- the alpha stage without a rast image ----

def _silhouette_args(name: str, pos, tri, resolution, topology_hash):
    pos = _check_pos(name, pos)
    height, width = _check_resolution(name, resolution, int(_check_tri(tri, pos.device).shape[0]))   # (the limits before a partner table is built)
    pos, tri, topo = _mesh_args(name, pos, tri, topology_hash)
    return pos, tri, height, width, topo


def _silhouette_forward(pos, tri, opp, glctx, height, width):
    """(alpha [B, H, W, 1], ids [B, H, W] int32, coverage masks) of tsamd_silhouette."""
    B, V = int(pos.shape[0]), int(pos.shape[1])
    alpha = torch.empty((B, height, width, 1), dtype=torch.float32, device=pos.device)
    ids = torch.empty((B, height, width), dtype=torch.int32, device=pos.device)
    masks = torch.empty((max(int(_lib.tsamd_pair_masks_bytes(B, height, width)), 8),), dtype=torch.uint8, device=pos.device)
    ws = glctx.workspace(B, V, height, width, pos.device)
    with _device_ctx(pos.device):
        _capi.check(_lib.tsamd_silhouette(pos.data_ptr(), B, V, tri.data_ptr(), int(tri.shape[0]), opp.data_ptr(), height, width, ws.data_ptr(),
                                          ids.data_ptr(), masks.data_ptr(), alpha.data_ptr(), _stream_ptr(pos.device)))
    return alpha, ids, masks


class _SilhouetteFunc(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, tri, opp, glctx, height, width, boost):
        alpha, ids, masks = _silhouette_forward(pos, tri, opp, glctx, height, width)
        ctx.save_for_backward(pos, tri, opp, ids, masks)
        ctx.boost = float(boost)
        return alpha

    @staticmethod
    def backward(ctx, grad_alpha):
        pos, tri, opp, ids, masks = ctx.saved_tensors
        B, V, H, W = int(pos.shape[0]), int(pos.shape[1]), int(ids.shape[1]), int(ids.shape[2])
        g = grad_alpha.contiguous()
        grad_pos = torch.empty_like(pos)
        with _device_ctx(pos.device):
            _capi.check(_lib.tsamd_silhouette_backward(pos.data_ptr(), B, V, tri.data_ptr(), int(tri.shape[0]), opp.data_ptr(), H, W, ids.data_ptr(),
                                                       masks.data_ptr(), g.data_ptr(), ctx.boost, grad_pos.data_ptr(), _stream_ptr(pos.device)))
        return grad_pos, None, None, None, None, None, None


def silhouette(glctx: RasterizeCudaContext, pos: torch.Tensor, tri: torch.Tensor, resolution, topology_hash=None, pos_gradient_boost: float = 1.0):
    """``alpha[B, H, W, 1]``: what ``antialias(clamp(rast[..., -1:], 0, 1), rast, pos, tri)`` of ``rasterize(glctx, pos, tri, resolution)``
    gives -- coverage 0 / 1 with the silhouette pixels blended -- without the ``rast`` image; differentiable w.r.t. ``pos``."""
    pos, tri, height, width, topo = _silhouette_args("silhouette", pos, tri, resolution, topology_hash)
    return _SilhouetteFunc.apply(pos, tri, topo.opp, glctx, height, width, float(pos_gradient_boost))


# An id-driven image term of the alpha stage's node, described once: the C entry point of its loss (``<entry>_backward`` and
# ``<entry>_workspace_bytes`` go with it), the channels of its image, and how many tensors it passes between ``ids_dev`` and the workspace
# -- its vertex attribute (the differentiable input) first, then its constants, in the entry points' order.
_ImageTerm = collections.namedtuple("_ImageTerm", "entry channels n_tensors")
_DEPTH_TERM = _ImageTerm("tsamd_depth_mse", 1, 4)        # world_pos; campos, target_depth, depth_mask
_NORMAL_TERM = _ImageTerm("tsamd_normal_mse", 3, 3)      # normals; target_normal, normal_mask


class _SilhouetteLossFunc(torch.autograd.Function):
    """One node for the image terms of the geometry stage: one rasterisation forward, the silhouette MSE and the losses of the ``terms``
    present from its ids; ``tsamd_silhouette_mse_backward`` followed by each term's backward with ``accumulate_pos=1`` backward -- each
    lands on what the one before wrote.  ``tensors``: the terms' tensors one after the other (:class:`_ImageTerm`)."""

    @staticmethod
    def forward(ctx, pos, tri, opp, glctx, height, width, target_alpha, boost, want_images, terms, *tensors):
        dev = pos.device
        B, V, T = int(pos.shape[0]), int(pos.shape[1]), int(tri.shape[0])
        alpha, ids, masks = _silhouette_forward(pos, tri, opp, glctx, height, width)
        n = alpha.numel()
        losses = [torch.empty((), dtype=torch.float32, device=dev) for _ in range(1 + len(terms))]
        make = torch.empty if n * T > 0 else torch.zeros         # (the calls write no image without triangles)
        images = [make((B, height, width, term.channels) if want_images else (0,), dtype=torch.float32, device=dev) for term in terms]
        sizes = [_lib.tsamd_silhouette_mse_workspace_bytes] + [getattr(_lib, term.entry + "_workspace_bytes") for term in terms]
        ws = torch.empty((max(int(size(n)) for size in sizes),), dtype=torch.uint8, device=dev)
        with _device_ctx(dev):
            stream = _stream_ptr(dev)
            _capi.check(_lib.tsamd_silhouette_mse(alpha.data_ptr(), target_alpha.data_ptr(), n, ws.data_ptr(), losses[0].data_ptr(), stream))
            at = 0
            for term, loss, image in zip(terms, losses[1:], images):
                own = tensors[at:at + term.n_tensors]
                _capi.check(getattr(_lib, term.entry)(_ptr(pos), B, V, _ptr(tri), T, height, width, _ptr(ids), *(_ptr(t) for t in own), ws.data_ptr(),
                                                      loss.data_ptr(), _ptr(image), stream))
                at += term.n_tensors
        ctx.save_for_backward(pos, tri, opp, ids, masks, alpha, target_alpha, *tensors)
        ctx.boost, ctx.terms = float(boost), terms
        ctx.mark_non_differentiable(alpha, *images)
        return (*losses, alpha, *images)

    @staticmethod
    def backward(ctx, *grads):
        pos, tri, opp, ids, masks, alpha, target_alpha, *tensors = ctx.saved_tensors
        B, V, T, H, W = int(pos.shape[0]), int(pos.shape[1]), int(tri.shape[0]), int(ids.shape[1]), int(ids.shape[2])
        g = [k.to(torch.float32).contiguous() for k in grads[:1 + len(ctx.terms)]]      # stay on the device: the kernels read them there
        grad_pos = torch.empty_like(pos)
        grad_tensors = [None] * len(tensors)
        with _device_ctx(pos.device):
            stream = _stream_ptr(pos.device)
            _capi.check(_lib.tsamd_silhouette_mse_backward(pos.data_ptr(), B, V, tri.data_ptr(), T, opp.data_ptr(), H, W, ids.data_ptr(), masks.data_ptr(),
                                                           alpha.data_ptr(), target_alpha.data_ptr(), g[0].data_ptr(), ctx.boost, grad_pos.data_ptr(), stream))
            at = 0
            for term, g_term in zip(ctx.terms, g[1:]):
                own = tensors[at:at + term.n_tensors]
                grad_tensors[at] = torch.empty_like(own[0])
                _capi.check(getattr(_lib, term.entry + "_backward")(_ptr(pos), B, V, _ptr(tri), T, H, W, _ptr(ids), *(_ptr(t) for t in own), g_term.data_ptr(),
                                                                    1, _ptr(grad_tensors[at]), _ptr(grad_pos), stream))
                at += term.n_tensors
        return (grad_pos,) + (None,) * 9 + tuple(grad_tensors)


def _silhouette_losses(glctx, pos, tri, topo, height, width, target_alpha, boost, return_images, terms, *tensors):
    """The losses of :class:`_SilhouetteLossFunc` -- the silhouette's, then one per term -- and, asked for, its detached images behind them."""
    out = _SilhouetteLossFunc.apply(pos, tri, topo.opp, glctx, height, width, target_alpha, float(boost), bool(return_images), terms, *tensors)
    n_losses = 1 + len(terms)
    return out[:n_losses] + tuple(image.detach() for image in out[n_losses:]) if return_images else out[:n_losses]


def silhouette_mse(glctx: RasterizeCudaContext, pos: torch.Tensor, tri: torch.Tensor, resolution, target: torch.Tensor, topology_hash=None,
                   pos_gradient_boost: float = 1.0, return_alpha: bool = False):
    """``mean((silhouette(...) - target) ** 2)`` as a 0-dim tensor (bitwise repeatable), differentiable w.r.t. ``pos`` without a
    gradient image; ``target`` is ``[B, H, W]`` or ``[B, H, W, 1]`` float32 and carries no gradient.  ``return_alpha=True``:
    ``(loss, alpha.detach())``."""
    pos, tri, height, width, topo = _silhouette_args("silhouette_mse", pos, tri, resolution, topology_hash)
    target = _check_cuda_f32("target", target)
    if target.device != pos.device:
        raise RuntimeError("tssplat_amd.dr.silhouette_mse: target and pos must live on the same device")
    shape = (int(pos.shape[0]), height, width)
    if tuple(target.shape) not in (shape, shape + (1,)):
        raise RuntimeError("tssplat_amd.dr.silhouette_mse: target must be [B, H, W] or [B, H, W, 1] of the image size")
    out = _silhouette_losses(glctx, pos, tri, topo, height, width, target.detach(), pos_gradient_boost, return_alpha, ())
    return out if return_alpha else out[0]


# the argument checks the id-driven terms (depth, normal) share; every result is detached unless it carries a gradient

def _scalar_image(name: str, label: str, t, pos, shape):
    t = _check_cuda_f32(label, t)
    if t.device != pos.device or tuple(t.shape) not in (shape, shape + (1,)):
        raise RuntimeError(f"tssplat_amd.dr.{name}: {label} must be [B, H, W] or [B, H, W, 1] of the image size, on the device of pos")
    return t.detach()


def _vertex_attribute(name: str, label: str, t, pos):
    V = int(pos.shape[1])
    t = _check_cuda_f32(label, t)
    if t.device != pos.device or tuple(t.shape) not in ((V, 3), (1, V, 3)):
        raise RuntimeError(f"tssplat_amd.dr.{name}: {label} must be [V, 3] or [1, V, 3] with V = {V} (the vertices of pos), on the device of pos")
    return t


def _camera_positions(name: str, campos, pos):
    B = int(pos.shape[0])
    campos = _check_cuda_f32("campos", campos)
    if campos.device != pos.device or tuple(campos.shape) != (B, 3):
        raise RuntimeError(f"tssplat_amd.dr.{name}: campos must be [B, 3] = [{B}, 3], on the device of pos")
    return campos.detach()


def silhouette_depth_mse(glctx: RasterizeCudaContext, pos: torch.Tensor, tri: torch.Tensor, resolution, target_alpha: torch.Tensor, world_pos: torch.Tensor,
                         campos: torch.Tensor, target_depth: torch.Tensor, depth_mask: torch.Tensor, topology_hash=None, pos_gradient_boost: float = 1.0,
                         return_images: bool = False):
    """``(alpha_loss, depth_loss)``, two 0-dim tensors (bitwise repeatable), from ONE rasterisation: ``alpha_loss`` is
    :func:`silhouette_mse`'s; ``depth_loss = mean((d * depth_mask - target_depth * depth_mask) ** 2)`` over ``B H W`` pixels with
    ``d = norm(interpolate(world_pos, rast, tri) - campos[:, None, None], dim=-1)`` of ``rasterize(glctx, pos, tri, resolution)`` --
    ``||campos||`` on background, as that chain gives -- without ``rast``, the interpolated image or a gradient image.  ``world_pos``
    is ``[V, 3]`` or ``[1, V, 3]``, ``campos`` ``[B, 3]``, the two targets and the mask ``[B, H, W]`` or ``[B, H, W, 1]`` float32;
    gradients flow to ``pos`` (the silhouette blends, and ``(u, v)`` as through ``rasterize``) and ``world_pos``, nowhere else.
    Without triangles ``depth_loss`` is 0.  ``return_images=True``: ``(alpha_loss, depth_loss, alpha.detach(), d.detach())``, both
    ``[B, H, W, 1]``."""
    name = "silhouette_depth_mse"
    pos, tri, height, width, topo = _silhouette_args(name, pos, tri, resolution, topology_hash)
    shape = (int(pos.shape[0]), height, width)
    images = [_scalar_image(name, label, t, pos, shape) for label, t in (("target_alpha", target_alpha), ("target_depth", target_depth), ("depth_mask", depth_mask))]
    world_pos = _vertex_attribute(name, "world_pos", world_pos, pos)
    campos = _camera_positions(name, campos, pos)
    return _silhouette_losses(glctx, pos, tri, topo, height, width, images[0], pos_gradient_boost, return_images, (_DEPTH_TERM,), world_pos, campos, images[1],
                              images[2])


def silhouette_normal_mse(glctx: RasterizeCudaContext, pos: torch.Tensor, tri: torch.Tensor, resolution, target_alpha: torch.Tensor, normals: torch.Tensor,
                          target_normal: torch.Tensor, normal_mask: torch.Tensor, *, depth=None, topology_hash=None, pos_gradient_boost: float = 1.0,
                          return_images: bool = False):
    """``(alpha_loss, normal_loss)``, or ``(alpha_loss, depth_loss, normal_loss)`` with ``depth=(world_pos, campos, target_depth,
    depth_mask)`` -- 0-dim tensors (bitwise repeatable) from ONE rasterisation and one autograd node.  ``alpha_loss`` is
    :func:`silhouette_mse`'s, ``depth_loss`` :func:`silhouette_depth_mse`'s (the shapes and checks of its arguments too);
    ``normal_loss = mean((n * normal_mask[..., None] - target_normal * normal_mask[..., None]) ** 2)`` over ``B H W 3`` values with
    ``n = interpolate(normals, rast, tri)`` of ``rasterize(glctx, pos, tri, resolution)`` -- 0 on background -- without ``rast``, the
    interpolated image or a gradient image.  ``normals`` is ``[V, 3]`` or ``[1, V, 3]`` (any 3-channel vertex attribute),
    ``target_normal`` ``[B, H, W, 3]``, ``normal_mask`` ``[B, H, W]`` or ``[B, H, W, 1]``, float32.  Gradients flow to ``pos`` (the
    silhouette blends, and ``(u, v)`` as through ``rasterize``), ``normals`` and ``world_pos``, nowhere else.  Without triangles
    ``normal_loss`` is 0.  ``return_images=True``: the detached images are appended in the same order -- ``alpha [B, H, W, 1]``,
    ``d [B, H, W, 1]`` with ``depth``, ``n [B, H, W, 3]``."""
    name = "silhouette_normal_mse"
    pos, tri, height, width, topo = _silhouette_args(name, pos, tri, resolution, topology_hash)
    shape = (int(pos.shape[0]), height, width)
    target_alpha = _scalar_image(name, "target_alpha", target_alpha, pos, shape)
    normal_mask = _scalar_image(name, "normal_mask", normal_mask, pos, shape)
    target_normal = _check_cuda_f32("target_normal", target_normal)
    if target_normal.device != pos.device or tuple(target_normal.shape) != shape + (3,):
        raise RuntimeError(f"tssplat_amd.dr.{name}: target_normal must be [B, H, W, 3] of the image size, on the device of pos")
    terms, tensors = (_NORMAL_TERM,), (_vertex_attribute(name, "normals", normals, pos), target_normal.detach(), normal_mask)
    if depth is not None:
        if not isinstance(depth, (tuple, list)) or len(depth) != 4:
            raise RuntimeError(f"tssplat_amd.dr.{name}: depth must be None or (world_pos, campos, target_depth, depth_mask)")
        terms = (_DEPTH_TERM,) + terms
        tensors = (_vertex_attribute(name, "world_pos", depth[0], pos), _camera_positions(name, depth[1], pos),
                   _scalar_image(name, "target_depth", depth[2], pos, shape), _scalar_image(name, "depth_mask", depth[3], pos, shape)) + tensors
    return _silhouette_losses(glctx, pos, tri, topo, height, width, target_alpha, pos_gradient_boost, return_images, terms, *tensors)


# ---- the colour stage under a blend plan ----

class BlendPlan:
    """The blends ``antialias(., rast, pos, tri)`` applies, for a FROZEN ``rast`` / ``pos`` / ``tri``, as data (:func:`plan_blends`).

    ``pix_point[B * H * W]`` int32: the row of a pixel's colour in ``color[N, 3]`` -- the order of ``positions_all[rast[..., 3] > 0]``
    -- or -1 on background; ``n_points = N``.  ``rec_dst / rec_src / rec_weight[n_blends]``: the blend records in extraction order
    (pair slot order: pixel-major, the pair with the right neighbour before the one with the upper neighbour, edges 0, 1, 2), pixel
    indices batch-wide.  ``dst_perm`` / ``src_perm``: the stable permutations that group the records by destination / by source;
    ``dst_pix[n_dst]`` and ``dst_ptr[n_dst + 1]`` (``src_pix``, ``src_ptr`` likewise) are the two CSR views, ``pix_dst[B * H * W]``
    the destination slot of a pixel or -1.  The remaining arrays are those views with the indices the kernels need next to them
    (include/tssplat_amd.h: tsamd_blend_plan)."""

    _STRUCT_FIELDS = ("pix_point", "pix_dst", "dst_ptr", "dst_src_pix", "dst_src_point", "dst_weight", "src_ptr", "src_dst_pix", "src_dst_slot",
                      "src_weight", "point_pix", "point_dst", "point_src")
    _OTHER_FIELDS = ("rec_dst", "rec_src", "rec_weight", "dst_perm", "src_perm", "dst_pix", "src_pix")

    def __init__(self, shape, n_points: int, **tensors):
        self.batch, self.height, self.width = (int(k) for k in shape)
        self.n_points = int(n_points)
        for name in self._STRUCT_FIELDS + self._OTHER_FIELDS:
            setattr(self, name, tensors[name])
        self.n_blends, self.n_dst, self.n_src = int(self.rec_dst.shape[0]), int(self.dst_pix.shape[0]), int(self.src_pix.shape[0])
        self.device = self.pix_point.device
        st = _capi.BlendPlanStruct()
        st.struct_size = _capi.C.sizeof(_capi.BlendPlanStruct)
        st.height, st.width, st.batch = self.height, self.width, self.batch
        st.n_points, st.n_blends, st.n_dst, st.n_src = self.n_points, self.n_blends, self.n_dst, self.n_src
        for name in self._STRUCT_FIELDS:
            t = getattr(self, name)
            setattr(st, name + "_dev", _ptr(t))
        self._struct = st

    def tensors(self) -> dict:
        return {name: getattr(self, name) for name in self._STRUCT_FIELDS + self._OTHER_FIELDS}

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.tensors().values())

    @property
    def shape(self):
        return (self.batch, self.height, self.width)


def _csr(keys: torch.Tensor, n_pixels: int):
    """Stable grouping of the records by ``keys`` (pixel indices): (perm, group pixels, ptr[n + 1] int32, slot per pixel or -1)."""
    dev = keys.device
    perm = torch.sort(keys, stable=True).indices
    pix, counts = torch.unique_consecutive(keys[perm], return_counts=True)
    ptr = torch.zeros(pix.shape[0] + 1, dtype=torch.int32, device=dev)
    ptr[1:] = torch.cumsum(counts, 0)
    slot = torch.full((n_pixels,), -1, dtype=torch.int32, device=dev)
    slot[pix.long()] = torch.arange(pix.shape[0], dtype=torch.int32, device=dev)
    return perm, pix, ptr, slot


def plan_blends(rast: torch.Tensor, pos: torch.Tensor, tri: torch.Tensor, topology_hash=None) -> BlendPlan:
    """The :class:`BlendPlan` of ``rast[B, H, W, 4]`` (as ``rasterize`` returned it), ``pos[B, V, 4]`` and ``tri``: the blends are
    exactly those ``antialias`` analyses on the same inputs (oracle/raster_oracle.py::antialias_events), weights
    ``float32(|t - 1/2|)``.  Runs once per plan: the records come from a count / scan / fill pass of the antialias analysis, the
    two groupings from stable sorts; it synchronises with the host (two sizes are read back)."""
    rast = _check_cuda_f32("rast", rast.detach())
    if rast.dim() != 4 or rast.shape[3] != 4:
        raise RuntimeError("tssplat_amd.dr.plan_blends: rast must be [B, H, W, 4]")
    pos = _check_pos("plan_blends", pos, rast.shape[0]).detach()
    if pos.device != rast.device:
        raise RuntimeError("tssplat_amd.dr.plan_blends: rast and pos must live on the same device")
    pos, tri, topo = _mesh_args("plan_blends", pos, tri, topology_hash, rast.device)
    B, H, W = (int(k) for k in rast.shape[:3])
    V, T, P = int(pos.shape[1]), int(tri.shape[0]), B * H * W
    if P >= 1 << 30:
        raise RuntimeError("tssplat_amd.dr.plan_blends: batch x height x width must stay below 2^30 pixels")
    dev = rast.device
    fg = rast[..., 3].reshape(-1) > 0
    rank = torch.cumsum(fg, 0, dtype=torch.int32)
    pix_point = torch.where(fg, rank - 1, torch.full_like(rank, -1))
    point_pix = torch.nonzero(fg).reshape(-1).to(torch.int32)
    n_points = int(point_pix.shape[0])
    counts = torch.empty(2 * P, dtype=torch.int32, device=dev)             # (zero-filled by the count call)
    prepared = torch.empty((max(int(_lib.tsamd_antialias_prepared_bytes(B, V, T, H, W)), 8),), dtype=torch.uint8, device=dev)
    args = (rast.data_ptr(), pos.data_ptr(), prepared.data_ptr(), tri.data_ptr(), topo.opp.data_ptr(), B, V, T, H, W)
    with _device_ctx(dev):
        stream = _stream_ptr(dev)
        _capi.check(_lib.tsamd_antialias_prepare(rast.data_ptr(), pos.data_ptr(), tri.data_ptr(), topo.opp.data_ptr(), None, B, V, T, H, W, prepared.data_ptr(),
                                                 stream))
        _capi.check(_lib.tsamd_shade_plan_count(*args, counts.data_ptr(), stream))
        ends = torch.cumsum(counts, 0, dtype=torch.int64)        # (scanned in 64 bits: the total is checked before it is narrowed)
        n_blends = int(ends[-1]) if P else 0
        if n_blends >= 1 << 31:
            raise RuntimeError(f"tssplat_amd.dr.plan_blends: {n_blends} blends; record offsets are 32-bit (at most 2^31 - 1)")
        offsets = (ends - counts).to(torch.int32)
        rec_dst = torch.empty(n_blends, dtype=torch.int32, device=dev)
        rec_src = torch.empty(n_blends, dtype=torch.int32, device=dev)
        rec_weight = torch.empty(n_blends, dtype=torch.float32, device=dev)
        _capi.check(_lib.tsamd_shade_plan_fill(*args, offsets.data_ptr(), n_blends, rec_dst.data_ptr(), rec_src.data_ptr(), rec_weight.data_ptr(), stream))
    dst_perm, dst_pix, dst_ptr, pix_dst = _csr(rec_dst, P)
    src_perm, src_pix, src_ptr, pix_src = _csr(rec_src, P)
    dst_src_pix, src_dst_pix = rec_src[dst_perm], rec_dst[src_perm]
    return BlendPlan((B, H, W), n_points, pix_point=pix_point, pix_dst=pix_dst, dst_ptr=dst_ptr, dst_src_pix=dst_src_pix,
                     dst_src_point=pix_point[dst_src_pix.long()], dst_weight=rec_weight[dst_perm], src_ptr=src_ptr, src_dst_pix=src_dst_pix,
                     src_dst_slot=pix_dst[src_dst_pix.long()], src_weight=rec_weight[src_perm], point_pix=point_pix,
                     point_dst=pix_dst[point_pix.long()], point_src=pix_src[point_pix.long()], rec_dst=rec_dst, rec_src=rec_src, rec_weight=rec_weight,
                     dst_perm=dst_perm, src_perm=src_perm, dst_pix=dst_pix, src_pix=src_pix)


def _shade_args(name: str, color, plan, background, target=None):
    if not isinstance(plan, BlendPlan):
        raise RuntimeError(f"tssplat_amd.dr.{name}: blend_plan must be a BlendPlan (dr.plan_blends)")
    color = _check_cuda_f32("color", color)
    background = _check_cuda_f32("background", background)
    if color.dim() != 2 or color.shape[1] != 3 or int(color.shape[0]) != plan.n_points:
        raise RuntimeError(f"tssplat_amd.dr.{name}: color must be [n_points, 3] with n_points = {plan.n_points} (the plan's foreground pixels), "
                           f"not {list(color.shape)}")
    if tuple(background.shape) != plan.shape + (3,):
        raise RuntimeError(f"tssplat_amd.dr.{name}: background must be [B, H, W, 3] = {list(plan.shape + (3,))} (the plan's batch and resolution), "
                           f"not {list(background.shape)}")
    if color.device != plan.device or background.device != plan.device:
        raise RuntimeError(f"tssplat_amd.dr.{name}: color, background and the plan must live on the same device")
    if target is None:
        return color, background
    if not isinstance(target, torch.Tensor) or not target.is_cuda or target.dtype != torch.float32 or target.device != plan.device:
        raise RuntimeError(f"tssplat_amd.dr.{name}: target must be a float32 GPU tensor on the plan's device")
    if tuple(target.shape[:3]) != plan.shape or target.dim() != 4 or target.shape[3] not in (3, 4):
        raise RuntimeError(f"tssplat_amd.dr.{name}: target must be [B, H, W, 3 or 4] of the plan's batch and resolution {list(plan.shape)}, "
                           f"not {list(target.shape)}")
    if not target.is_contiguous():
        raise RuntimeError(f"tssplat_amd.dr.{name}: target must be contiguous (a four-channel target is read with its channel stride: pass it whole, "
                           "not a slice)")
    return color, background, target.detach()


class _ShadeFunc(torch.autograd.Function):
    @staticmethod
    def forward(ctx, color, plan, background):
        out = torch.empty(plan.shape + (3,), dtype=torch.float32, device=color.device)
        with _device_ctx(color.device):
            _capi.check(_lib.tsamd_shade(plan._struct, color.data_ptr(), background.data_ptr(), out.data_ptr(), _stream_ptr(color.device)))
        ctx.plan = plan
        return out

    @staticmethod
    def backward(ctx, grad_out):
        plan = ctx.plan
        g = grad_out.contiguous()
        grad_color = torch.empty((plan.n_points, 3), dtype=torch.float32, device=g.device)
        with _device_ctx(g.device):
            _capi.check(_lib.tsamd_shade_backward(plan._struct, g.data_ptr(), grad_color.data_ptr(), _stream_ptr(g.device)))
        return grad_color, None, None


def shade(color: torch.Tensor, blend_plan: BlendPlan, background: torch.Tensor) -> torch.Tensor:
    """``[B, H, W, 3]``: ``antialias(lerp(background, scatter(color), mask), rast, pos, tri)`` of the plan's ``rast`` / ``pos`` /
    ``tri`` -- ``color[N, 3]`` in the order of ``positions_all[rast[..., 3] > 0]``, ``background[B, H, W, 3]`` -- in one pass, one
    lane per pixel: ``out = c_p + sum w (c_src - c_p)`` over the pixel's blends in the plan's order.  Differentiable w.r.t.
    ``color`` only (the plan is frozen: there is no gradient w.r.t. positions); the backward writes ``[N, 3]`` without atomics."""
    color, background = _shade_args("shade", color, blend_plan, background)
    return _ShadeFunc.apply(color, blend_plan, background.detach())


class _ShadeL1Func(torch.autograd.Function):
    @staticmethod
    def forward(ctx, color, plan, background, target, want_image):
        dev = color.device
        loss = torch.empty((), dtype=torch.float32, device=dev)
        image = torch.empty(plan.shape + (3,) if want_image else (0,), dtype=torch.float32, device=dev)
        need_grad = ctx.needs_input_grad[0]
        point_sign = torch.empty((plan.n_points, 3), dtype=torch.float32, device=dev) if need_grad else None
        dst_sign = torch.empty((plan.n_dst, 3), dtype=torch.float32, device=dev) if need_grad else None
        ws = torch.empty((int(_lib.tsamd_shade_l1_workspace_bytes(plan.batch * plan.height * plan.width)),), dtype=torch.uint8, device=dev)
        with _device_ctx(dev):
            _capi.check(_lib.tsamd_shade_l1(plan._struct, color.data_ptr(), background.data_ptr(), target.data_ptr(), int(target.shape[3]), ws.data_ptr(),
                                            loss.data_ptr(), _ptr(image), _ptr(point_sign), _ptr(dst_sign), _stream_ptr(dev)))
        ctx.plan = plan
        if need_grad:
            ctx.save_for_backward(point_sign, dst_sign)
        ctx.mark_non_differentiable(image)
        return loss, image

    @staticmethod
    def backward(ctx, grad_loss, _grad_image):
        plan = ctx.plan
        point_sign, dst_sign = ctx.saved_tensors
        g = grad_loss.to(torch.float32).contiguous()            # stays on the device: the kernel reads it there
        grad_color = torch.empty((plan.n_points, 3), dtype=torch.float32, device=g.device)
        with _device_ctx(g.device):
            _capi.check(_lib.tsamd_shade_l1_backward(plan._struct, _ptr(point_sign), _ptr(dst_sign), g.data_ptr(), grad_color.data_ptr(), _stream_ptr(g.device)))
        return grad_color, None, None, None, None


def shade_l1(color: torch.Tensor, blend_plan: BlendPlan, background: torch.Tensor, target: torch.Tensor, return_image: bool = False):
    """``torch.nn.L1Loss()(shade(color, blend_plan, background)[..., :3], target[..., :3])`` as a 0-dim float32 tensor, bitwise
    repeatable, without the image: ``target`` is ``[B, H, W, 3]`` or ``[B, H, W, 4]`` (contiguous; of four channels the first three
    are read in place) and carries no gradient.  Differentiable w.r.t. ``color``: the forward keeps ``sign(out - target)`` per point
    and per blended pixel (``sign(0) = 0``), the backward scales them by the device-side ``grad_loss / n`` -- no gradient image.
    ``return_image=True``: ``(loss, image)`` with the detached image the loss was taken of."""
    color, background, target = _shade_args("shade_l1", color, blend_plan, background, target)
    loss, image = _ShadeL1Func.apply(color, blend_plan, background.detach(), target, bool(return_image))
    return (loss, image.detach()) if return_image else loss


_TEX_FILTERS = {"nearest": _capi.TSAMD_TEX_FILTER_NEAREST, "linear": _capi.TSAMD_TEX_FILTER_LINEAR}                  # include/tssplat_amd.h
_TEX_BOUNDARIES = {"wrap": _capi.TSAMD_TEX_BOUNDARY_WRAP, "clamp": _capi.TSAMD_TEX_BOUNDARY_CLAMP, "zero": _capi.TSAMD_TEX_BOUNDARY_ZERO}


class _TextureFunc(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tex, uv, filter_mode, boundary_mode):
        TB, TH, TW, Cn = (int(k) for k in tex.shape)
        B, H, W = int(uv.shape[0]), int(uv.shape[1]), int(uv.shape[2])
        out = torch.empty((B, H, W, Cn), dtype=torch.float32, device=uv.device)
        with _device_ctx(uv.device):
            _capi.check(_lib.tsamd_texture(tex.data_ptr(), TB, TH, TW, Cn, uv.data_ptr(), B, H, W, filter_mode, boundary_mode, out.data_ptr(),
                                           _stream_ptr(uv.device)))
        ctx.save_for_backward(tex, uv)
        ctx.modes = (filter_mode, boundary_mode)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        tex, uv = ctx.saved_tensors
        filter_mode, boundary_mode = ctx.modes
        TB, TH, TW, Cn = (int(k) for k in tex.shape)
        B, H, W = int(uv.shape[0]), int(uv.shape[1]), int(uv.shape[2])
        g = grad_out.contiguous()
        grad_tex = torch.empty_like(tex) if ctx.needs_input_grad[0] else None          # (zero-filled by the call)
        grad_uv = torch.empty_like(uv) if ctx.needs_input_grad[1] and filter_mode == _TEX_FILTERS["linear"] else None
        if grad_tex is not None or grad_uv is not None:
            with _device_ctx(uv.device):
                _capi.check(_lib.tsamd_texture_backward(tex.data_ptr(), TB, TH, TW, Cn, uv.data_ptr(), B, H, W, filter_mode, boundary_mode, g.data_ptr(),
                                                        _ptr(grad_tex), _ptr(grad_uv), _stream_ptr(uv.device)))
        return grad_tex, grad_uv, None, None


def texture(tex: torch.Tensor, uv: torch.Tensor, uv_da=None, mip_level_bias=None, mip=None, filter_mode: str = "auto",
            boundary_mode: str = "wrap", max_mip_level=None):
    """``dr.texture``: ``out[B, h, w, C]`` = ``tex[1 or B, H, W, C]`` sampled at ``uv[B, h, w, 2]``, nvdiffrast's names and
    argument order.  ``filter_mode`` ``'nearest'`` or ``'linear'`` (``'auto'`` = ``'linear'``: there are no mipmaps to choose);
    ``boundary_mode`` ``'wrap'`` (a true modulo), ``'clamp'`` or ``'zero'``.  ``x = u W - 0.5``, ``y = v H - 0.5``, no flip;
    linear filtering takes the taps at ``floor(x)``, ``floor(x) + 1`` and likewise in ``y`` with the fractional parts as
    weights, nearest takes texel ``floor(u W)``, ``floor(v H)`` (tests/texture_oracle.py; PARITY UNPINNED against nvdiffrast).

    Differentiable w.r.t. ``tex`` (summed over the batch when ``tex`` has batch 1; float atomics, so the last bits are not
    repeatable from run to run) and, for ``'linear'``, w.r.t. ``uv`` from the taps actually used; ``'nearest'`` gives ``uv``
    no gradient (``None``).  ``uv_da``, ``mip_level_bias``, ``mip``, ``max_mip_level``, the ``'linear-mipmap-*'`` filters and
    ``boundary_mode='cube'`` are not part of this slice and raise."""
    if uv_da is not None or mip_level_bias is not None or mip is not None or max_mip_level is not None:
        raise NotImplementedError("tssplat_amd.dr.texture: uv_da / mip_level_bias / mip / max_mip_level (mipmaps) are not part of this slice")
    if filter_mode == "auto":
        filter_mode = "linear"
    if filter_mode in ("linear-mipmap-nearest", "linear-mipmap-linear"):
        raise NotImplementedError(f"tssplat_amd.dr.texture: filter_mode={filter_mode!r} (mipmaps) is not part of this slice")
    if boundary_mode == "cube":
        raise NotImplementedError("tssplat_amd.dr.texture: boundary_mode='cube' (cube maps) is not part of this slice")
    if filter_mode not in _TEX_FILTERS:
        raise ValueError(f"tssplat_amd.dr.texture: unknown filter_mode {filter_mode!r}")
    if boundary_mode not in _TEX_BOUNDARIES:
        raise ValueError(f"tssplat_amd.dr.texture: unknown boundary_mode {boundary_mode!r}")
    tex = _check_cuda_f32("tex", tex)
    uv = _check_cuda_f32("uv", uv)
    if uv.dim() != 4 or uv.shape[3] != 2:
        raise RuntimeError("tssplat_amd.dr.texture: uv must be [B, h, w, 2]")
    if tex.dim() != 4 or tex.shape[0] not in (1, uv.shape[0]) or min(tex.shape[1:]) < 1:
        raise RuntimeError("tssplat_amd.dr.texture: tex must be [1 or B, H, W, C] with H, W, C >= 1")
    if tex.device != uv.device:
        raise RuntimeError("tssplat_amd.dr.texture: tex and uv must live on the same device")
    return _TextureFunc.apply(tex, uv, _TEX_FILTERS[filter_mode], _TEX_BOUNDARIES[boundary_mode])
