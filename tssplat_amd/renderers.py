"""Mirror of ``MeshRasterizer`` (/root/reference/renderers/mesh_rasterizer.py:20-166) over this package's operators -- the
caller of SURVEY 8(f) rows 2 and 4: geometry forward (energy + surface gather), ``transform_pos``, ``dr.rasterize``,
``dr.antialias`` of the alpha image, and the optional colour / normal / depth branches through ``dr.interpolate``.

Same ``forward`` arguments and output keys (``"shaded"``, ``"geo_regularization"``, ``"n"``, ``"d"``) as the reference, so that
trainer.py:81-130 reads the same against either.  Host logic only: every tensor operation that is not one of this package's
kernels is the torch call the reference itself makes (clamp, lerp, masked assignment, norm).  ``export`` keeps the reference's
signature and file names but not its route (trimesh / pymeshlab / xatlas): the colour field is baked into this package's own
closed-form atlas (tssplat_amd/atlas.py).  Not mirrored: the reference's structured-config plumbing (``context_type="gl"`` is
served by the same HIP kernels as ``"cuda"``; the two ``Config`` fields are keyword arguments).
"""
from __future__ import annotations

import os
from typing import Optional

import numpy as np
import torch

from . import atlas, dr

__all__ = ["MeshRasterizer", "ViewPlan"]


class ViewPlan:
    """What the colour branch of :meth:`MeshRasterizer.forward` derives from a frozen surface under a fixed batch of views:
    ``pos_clip``, ``rast_out``, the foreground ``selector`` and the material's point plan for the foreground points, in the
    selector's order.  Built by :meth:`MeshRasterizer.plan_views`."""

    def __init__(self, mvp, resolution: int, pos_clip, rast_out, selector, point_plan, tri=None):
        self.mvp, self.resolution = mvp, int(resolution)
        self.pos_clip, self.rast_out, self.selector, self.point_plan = pos_clip, rast_out, selector, point_plan
        self.tri = tri
        self._blend_plan = None

    @property
    def blend_plan(self) -> "dr.BlendPlan":
        """The blends of ``dr.antialias`` on this plan's ``rast_out`` / ``pos_clip`` (``dr.plan_blends``), built on first use: what
        ``MeshRasterizer(fused_shade=True)`` and ``MeshRasterizer.shade_loss`` run on."""
        if self._blend_plan is None:
            if self.tri is None:
                raise RuntimeError("ViewPlan.blend_plan: the plan carries no triangle list (build it with MeshRasterizer.plan_views)")
            self._blend_plan = dr.plan_blends(self.rast_out, self.pos_clip, self.tri)
        return self._blend_plan

    @property
    def n_points(self) -> int:
        return self.point_plan.n_points


class MeshRasterizer(torch.nn.Module):
    def __init__(self, geometry: torch.nn.Module, materials: Optional[torch.nn.Module] = None, context_type: str = "cuda", is_orhto: bool = False,
                 fused_silhouette: bool = False, fused_shade: bool = False):
        super().__init__()
        # opt-in: forward(only_alpha=False, view_plan=plan) takes the image from dr.shade on the plan's blend plan (no alpha
        # antialias, no zero image, no masked scatter, no lerp, no per-call pair analysis); without a view plan it changes nothing
        self.fused_shade = bool(fused_shade)
        # opt-in: forward(only_alpha=True) without fit_normal / fit_depth takes alpha from dr.silhouette (no rast image)
        self.fused_silhouette = bool(fused_silhouette)
        if context_type not in ("cuda", "gl"):                       # mesh_rasterizer.py:33-38
            raise ValueError("Invalid context type")
        self.is_orhto = bool(is_orhto)                               # (the reference's spelling, mesh_rasterizer.py:24)
        self.glctx = dr.RasterizeCudaContext() if context_type == "cuda" else dr.RasterizeGLContext()   # (both are the HIP kernels)
        self.geometry = geometry
        self.materials = materials
        self.device = geometry.device
        n_surface = int(self.geometry.surface_vid.shape[0])
        self.ones_surface_v = torch.ones([n_surface, 1], device=self.device)      # mesh_rasterizer.py:49-53
        self.zeros_surface_v = torch.zeros([n_surface, 1], device=self.device)
        self.tri_hash = None                                         # mesh_rasterizer.py:55: the topology is rebuilt (here: cached) per call

    def transform_pos(self, mtx, pos, is_vec: bool = False):
        """``[pos, 1 | 0] @ mtx^T`` per view (mesh_rasterizer.py:57-78)."""
        t_mtx = torch.from_numpy(mtx).to(self.device) if isinstance(mtx, np.ndarray) else mtx.to(self.device)
        posw = torch.cat([pos, self.zeros_surface_v if is_vec else self.ones_surface_v], dim=1)
        res = torch.matmul(posw, t_mtx.transpose(1, 2))
        if not is_vec and self.is_orhto:
            res = res.clone()
            res[..., 2] /= 6
        return res

    def plan_views(self, mvp: torch.Tensor, resolution: int, iter_num: int = 0) -> ViewPlan:
        """Plans the texture stage's colour branch for one batch of views over FROZEN geometry: geometry, ``transform_pos``,
        ``dr.rasterize`` and ``dr.interpolate`` run once, without gradients, and the material sorts the foreground points once
        (``materials.plan_points``).  ``forward(..., view_plan=plan)`` then skips all four and the boolean compaction, and the
        grid's dL/dparams is the planned route's: no sort, no float atomics.

        A plan belongs to one point set in one order: these views, in this order, at this resolution.  A trainer whose loader
        reshuffles the views every iteration keeps one plan per batch composition, or feeds the views in a fixed order.
        Raises unless the geometry is frozen (``geometry.tet_v`` a buffer, not a Parameter) and the material offers
        ``plan_points``."""
        if isinstance(getattr(self.geometry, "tet_v", None), torch.nn.Parameter):
            raise RuntimeError("MeshRasterizer.plan_views: the geometry is being optimised (tet_v is a Parameter); a view plan "
                               "needs a frozen surface (optimize_geo=False)")
        if self.materials is None or not hasattr(self.materials, "plan_points"):
            raise RuntimeError("MeshRasterizer.plan_views: materials must offer plan_points (ExplicitMaterial does)")
        with torch.no_grad():
            data = self.geometry(iter_num=iter_num)
            tri = data.t_pos_idx
            pos_clip = self.transform_pos(mvp, data.v_pos).contiguous()
            rast_out, _ = dr.rasterize(self.glctx, pos_clip, tri, resolution=[resolution, resolution], grad_db=False)
            selector = rast_out[..., -1] > 0
            positions_all, _ = dr.interpolate(data.v_pos[None, ...], rast_out, tri)
            point_plan = self.materials.plan_points(positions_all[selector])
        return ViewPlan(mvp, resolution, pos_clip, rast_out, selector, point_plan, tri=tri)

    def _geometry_forward(self, iter_num: int, permute_surface_scheduler=None):
        """The geometry forward of one iteration, with the surface permutation the scheduler asks for (mesh_rasterizer.py:90-94)."""
        geo_input = {"iter_num": iter_num}
        if permute_surface_scheduler is not None:
            permute_dev = permute_surface_scheduler(iter_num)
            if permute_dev is not None:
                geo_input["permute_surface_v"] = True
                geo_input["permute_surface_v_dev"] = permute_dev
        return self.geometry(**geo_input)

    def forward(self, mvp: torch.Tensor, only_alpha: bool, iter_num: int, resolution: int, permute_surface_scheduler=None,
                fit_normal: bool = False, fit_depth: bool = False, background: Optional[torch.Tensor] = None,
                campos: Optional[torch.Tensor] = None, view_plan: Optional[ViewPlan] = None):
        if view_plan is not None:
            return self._forward_planned(view_plan, only_alpha, iter_num, resolution, permute_surface_scheduler, fit_normal, fit_depth,
                                         background, campos)
        data = self._geometry_forward(iter_num, permute_surface_scheduler)
        res = [resolution, resolution]
        tri = data.t_pos_idx

        pos_clip = self.transform_pos(mvp, data.v_pos).contiguous()
        if self.fused_silhouette and only_alpha and not fit_normal and not fit_depth:      # (either of the two needs rast_out)
            shaded = dr.silhouette(self.glctx, pos_clip, tri, res, topology_hash=self.tri_hash, pos_gradient_boost=1.0)
            return {"shaded": shaded, "geo_regularization": data.smooth_barrier_energy}
        rast_out, _ = dr.rasterize(self.glctx, pos_clip, tri, resolution=res, grad_db=False)
        # mesh_rasterizer.py:106-108.  The id channel carries no gradient (a triangle id + 1 is >= 1: the clamp is flat there, and
        # rasterize's backward ignores that channel anyway), so it is detached here: autograd would otherwise run the clamp's and
        # the slice's backward and a rasterize backward over all B x H x W pixels to deliver zeros -- 0.3 ms of 2 ms at 120 views.
        alpha = torch.clamp(rast_out[..., -1:].detach(), 0, 1)
        alpha = dr.antialias(alpha.contiguous(), rast_out, pos_clip, tri, topology_hash=self.tri_hash, pos_gradient_boost=1.0)

        shaded = alpha
        if not only_alpha:                                           # mesh_rasterizer.py:111-133
            assert self.materials is not None
            assert background is not None
            mask = rast_out[..., -1:] > 0
            selector = mask[..., 0]
            positions_all, _ = dr.interpolate(data.v_pos[None, ...], rast_out, tri)
            color = self.materials(positions=positions_all[selector])["color"]
            gb_fg = torch.zeros(rast_out.shape[0], res[0], res[0], 3, device=self.device)
            gb_fg[selector] = color
            gb_mat = torch.lerp(background, gb_fg, mask.float())
            shaded = dr.antialias(gb_mat.contiguous(), rast_out, pos_clip, tri, topology_hash=self.tri_hash, pos_gradient_boost=1.0)

        out = {"shaded": shaded, "geo_regularization": data.smooth_barrier_energy}

        if fit_normal:                                               # mesh_rasterizer.py:138-148
            v_s = data._compute_vertex_normal()[None, ...]
            scale = torch.tensor([1, 1, -1], dtype=torch.float32, device=self.device)[None, None, :]
            v_n, _ = dr.interpolate((v_s * scale).contiguous(), rast_out, tri)
            out["n"] = v_n

        if fit_depth:                                                # mesh_rasterizer.py:150-161
            assert campos is not None
            world_pos, _ = dr.interpolate(data.v_pos[None, ...], rast_out, tri)
            out["d"] = torch.norm(world_pos - campos[:, None, None, :], dim=-1, keepdim=True)
        return out

    def silhouette_loss(self, mvp: torch.Tensor, target_alpha: torch.Tensor, iter_num: int, resolution: int, permute_surface_scheduler=None):
        """The alpha stage's render and image loss in one: ``{"img_loss", "geo_regularization", "shaded"}`` with ``img_loss`` the
        plain mean squared error of ``forward(mvp, only_alpha=True, ...)["shaded"]`` against ``target_alpha`` (``[B, H, W]`` or
        ``[B, H, W, 1]``; the caller applies the trainer's weights) through ``dr.silhouette_mse`` -- no ``rast`` image, no
        gradient image -- and ``shaded`` detached."""
        data = self._geometry_forward(iter_num, permute_surface_scheduler)
        pos_clip = self.transform_pos(mvp, data.v_pos).contiguous()
        loss, shaded = dr.silhouette_mse(self.glctx, pos_clip, data.t_pos_idx, [resolution, resolution], target_alpha, topology_hash=self.tri_hash,
                                         pos_gradient_boost=1.0, return_alpha=True)
        return {"img_loss": loss, "geo_regularization": data.smooth_barrier_energy, "shaded": shaded}

    def silhouette_depth_loss(self, mvp: torch.Tensor, target_alpha: torch.Tensor, campos: torch.Tensor, target_depth: torch.Tensor, iter_num: int,
                              resolution: int, permute_surface_scheduler=None, depth_mask: Optional[torch.Tensor] = None):
        """The geometry stage's render and BOTH image losses in one (trainer.py:96-115 with ``fit_depth``):
        ``{"img_loss", "depth_loss", "geo_regularization", "shaded", "d"}`` with ``img_loss`` as :meth:`silhouette_loss` gives it and
        ``depth_loss`` the plain mean squared error of ``forward(..., only_alpha=True, fit_depth=True, campos=campos)["d"][..., -1] *
        depth_mask`` against ``target_depth * depth_mask`` through ``dr.silhouette_depth_mse`` -- one rasterisation, no ``rast`` image,
        no interpolated image, no gradient image.  ``depth_mask`` defaults to ``target_alpha`` (the trainer's ``color_ref[..., -1]``);
        the caller applies the trainer's weights; ``shaded`` and ``d`` are detached."""
        data = self._geometry_forward(iter_num, permute_surface_scheduler)
        pos_clip = self.transform_pos(mvp, data.v_pos).contiguous()
        mask = target_alpha if depth_mask is None else depth_mask
        img_loss, depth_loss, shaded, d = dr.silhouette_depth_mse(self.glctx, pos_clip, data.t_pos_idx, [resolution, resolution], target_alpha, data.v_pos,
                                                                  campos.to(self.device), target_depth, mask, topology_hash=self.tri_hash,
                                                                  pos_gradient_boost=1.0, return_images=True)
        return {"img_loss": img_loss, "depth_loss": depth_loss, "geo_regularization": data.smooth_barrier_energy, "shaded": shaded, "d": d}

    def silhouette_normal_loss(self, mvp: torch.Tensor, target_alpha: torch.Tensor, target_normal: torch.Tensor, iter_num: int, resolution: int,
                               permute_surface_scheduler=None, normal_mask: Optional[torch.Tensor] = None, campos: Optional[torch.Tensor] = None,
                               target_depth: Optional[torch.Tensor] = None, depth_mask: Optional[torch.Tensor] = None):
        """The geometry stage's render and its image losses with the normal term, in one:
        ``{"img_loss", "normal_loss", "geo_regularization", "shaded", "n"}`` with ``img_loss`` as :meth:`silhouette_loss` gives it and
        ``normal_loss`` the plain mean squared error of ``forward(..., only_alpha=True, fit_normal=True)["n"] * normal_mask[..., None]``
        against ``target_normal * normal_mask[..., None]`` (``target_normal`` ``[B, H, W, 3]``) through ``dr.silhouette_normal_mse`` -- one
        rasterisation, no ``rast`` image, no interpolated image, no gradient image.  The vertex attribute is ``forward``'s
        (mesh_rasterizer.py:138-148): ``data._compute_vertex_normal() * [1, 1, -1]``, so autograd carries its gradient through the
        vertex-normal operator into ``tet_v``.  With ``campos`` and ``target_depth`` the depth term of :meth:`silhouette_depth_loss`
        comes from the same rasterisation: ``"depth_loss"`` and ``"d"`` are added.  Both masks default to ``target_alpha``; the caller
        applies the trainer's weights; ``shaded``, ``n`` and ``d`` are detached."""
        if (campos is None) != (target_depth is None):
            raise RuntimeError("MeshRasterizer.silhouette_normal_loss: the depth term needs both campos and target_depth")
        data = self._geometry_forward(iter_num, permute_surface_scheduler)
        pos_clip = self.transform_pos(mvp, data.v_pos).contiguous()
        scale = torch.tensor([1, 1, -1], dtype=torch.float32, device=self.device)[None, :]
        v_s = (data._compute_vertex_normal() * scale).contiguous()
        depth = None
        if campos is not None:
            depth = (data.v_pos, campos.to(self.device), target_depth, target_alpha if depth_mask is None else depth_mask)
        got = dr.silhouette_normal_mse(self.glctx, pos_clip, data.t_pos_idx, [resolution, resolution], target_alpha, v_s, target_normal,
                                       target_alpha if normal_mask is None else normal_mask, depth=depth, topology_hash=self.tri_hash,
                                       pos_gradient_boost=1.0, return_images=True)
        names = ("img_loss", "normal_loss", "shaded", "n") if depth is None else ("img_loss", "depth_loss", "normal_loss", "shaded", "d", "n")
        return {**dict(zip(names, got)), "geo_regularization": data.smooth_barrier_energy}

    def shade_loss(self, view_plan: ViewPlan, background: torch.Tensor, target: torch.Tensor, iter_num: int, permute_surface_scheduler=None):
        """The colour stage's render and image loss in one, under a view plan: ``{"img_loss", "geo_regularization", "shaded"}`` with
        ``img_loss`` the plain ``L1Loss`` of ``forward(..., view_plan=view_plan)["shaded"][..., :3]`` against ``target[..., :3]``
        (``[B, H, W, 3]`` or ``[B, H, W, 4]``; the caller applies the trainer's weights) through ``dr.shade_l1`` -- no image-sized
        temporary besides ``shaded`` itself, which is detached."""
        self._check_planned(view_plan, False, iter_num, view_plan.resolution, permute_surface_scheduler)
        assert self.materials is not None
        data = self.geometry(iter_num=iter_num)
        color = self.materials(positions=view_plan.point_plan)["color"].float()
        loss, shaded = dr.shade_l1(color, view_plan.blend_plan, background, target, return_image=True)
        return {"img_loss": loss, "geo_regularization": data.smooth_barrier_energy, "shaded": shaded}

    @staticmethod
    def _check_planned(plan: ViewPlan, only_alpha, iter_num, resolution, permute_surface_scheduler):
        if only_alpha:
            raise RuntimeError("MeshRasterizer.forward: view_plan with only_alpha=True (a view plan is the colour branch's)")
        if permute_surface_scheduler is not None and permute_surface_scheduler(iter_num) is not None:
            raise RuntimeError("MeshRasterizer.forward: view_plan while permute_surface_scheduler perturbs the surface at "
                               f"iteration {iter_num}: the surface would move under the plan")
        if int(resolution) != plan.resolution:
            raise RuntimeError(f"MeshRasterizer.forward: view_plan was built at resolution {plan.resolution}, not {resolution}")

    def _forward_planned(self, plan: ViewPlan, only_alpha, iter_num, resolution, permute_surface_scheduler, fit_normal, fit_depth,
                         background, campos):
        """``forward`` with a :class:`ViewPlan`: the geometry forward still runs (``geo_regularization``), alpha and both
        ``antialias`` calls are as without a plan, the colour comes from the material's point plan.  ``fused_shade``: the image
        comes from ``dr.shade`` on the plan's blend plan instead."""
        self._check_planned(plan, only_alpha, iter_num, resolution, permute_surface_scheduler)
        assert self.materials is not None
        assert background is not None
        data = self.geometry(iter_num=iter_num)
        tri = data.t_pos_idx
        pos_clip, rast_out = plan.pos_clip, plan.rast_out
        if self.fused_shade:
            shaded = dr.shade(self.materials(positions=plan.point_plan)["color"].float(), plan.blend_plan, background)
        else:
            alpha = torch.clamp(rast_out[..., -1:], 0, 1)
            alpha = dr.antialias(alpha.contiguous(), rast_out, pos_clip, tri, topology_hash=self.tri_hash, pos_gradient_boost=1.0)

            color = self.materials(positions=plan.point_plan)["color"]
            gb_fg = torch.zeros(rast_out.shape[0], plan.resolution, plan.resolution, 3, device=self.device)
            gb_fg[plan.selector] = color
            gb_mat = torch.lerp(background, gb_fg, plan.selector[..., None].float())
            shaded = dr.antialias(gb_mat.contiguous(), rast_out, pos_clip, tri, topology_hash=self.tri_hash, pos_gradient_boost=1.0)
        out = {"shaded": shaded, "geo_regularization": data.smooth_barrier_energy}

        if fit_normal:
            v_s = data._compute_vertex_normal()[None, ...]
            scale = torch.tensor([1, 1, -1], dtype=torch.float32, device=self.device)[None, None, :]
            v_n, _ = dr.interpolate((v_s * scale).contiguous(), rast_out, tri)
            out["n"] = v_n
        if fit_depth:
            assert campos is not None
            world_pos, _ = dr.interpolate(data.v_pos[None, ...], rast_out, tri)
            out["d"] = torch.norm(world_pos - campos[:, None, None, :], dim=-1, keepdim=True)
        return out

    def export(self, path: str, folder: str, texture_res: int = 1024):
        """``renderer.export(f"{cfg.output_path}/final", "material")`` (trainer.py, mesh_rasterizer.py:165): writes
        ``exported_surface.obj``, ``.mtl`` and ``.png`` under ``path/folder`` -- the surface ``tet_v[surface_vid]`` /
        ``surface_fid`` with per-wedge UVs of the closed-form atlas at ``texture_res`` and ``self.materials`` baked into it
        (:mod:`tssplat_amd.atlas`; unowned texels stay black, there is no inpainting)."""
        assert self.materials is not None
        out_dir = os.path.join(path, folder)
        os.makedirs(out_dir, exist_ok=True)
        with torch.no_grad():
            v_pos = self.geometry.tet_v.detach()[self.geometry.surface_vid.long()].contiguous()
            t_pos_idx = self.geometry.surface_fid
            # (geometry.uv / uv_idx are this atlas at the geometry's default resolution; the atlas depends on texture_res)
            v_tex, t_tex_idx = atlas.atlas_uv(int(t_pos_idx.shape[0]), texture_res)
            tex = atlas.bake_material(self.materials, v_pos, t_pos_idx, texture_res)
        atlas.write_textured_obj(out_dir, "exported_surface", v_pos, t_pos_idx, v_tex, t_tex_idx, tex)

    def export_merged(self, path: str, folder: str, texture_res: Optional[int] = None, grid: int = 128, fill: str = "none", simplify=None,
                      smooth=None):
        """Writes ``merged_surface.obj``, ``.mtl`` and ``.png`` under ``path/folder``: the union of the geometry's tets as one closed
        surface (:func:`tssplat_amd.merge.merge_tets` at ``grid`` nodes per axis) with ``self.materials`` baked into the
        closed-form atlas.  The colour field is a function of position, so the bake is the one of :meth:`export`, unchanged.
        ``texture_res=None``: the smallest power of two >= 1024 whose atlas holds the triangles (marching tetrahedra makes many).
        ``fill``: as in ``merge_tets`` -- ``"cavities"`` and ``"outer"`` spare the atlas the triangles nobody can see.
        ``simplify=k``: the surface is clustered on ``grid // k`` cells per axis before the bake (``merge_tets(simplify=k)``); fewer
        triangles, so ``texture_res=None`` picks a smaller atlas by itself.  ``smooth=n``: ``n`` iterations of
        :func:`tssplat_amd.smooth.smooth` on the surface before the bake (``merge_tets(smooth=n)``); the faces, and so the atlas layout,
        are the same as without.  Returns the ``MergedSurface``."""
        from . import merge
        assert self.materials is not None
        out_dir = os.path.join(path, folder)
        os.makedirs(out_dir, exist_ok=True)
        with torch.no_grad():
            merged = merge.merge_tets(self.geometry.tet_v.detach(), self.geometry.tet_elem, grid=grid, fill=fill, simplify=simplify, smooth=smooth)
            n_tri = int(merged.faces.shape[0])
            if n_tri == 0:
                raise ValueError("MeshRasterizer.export_merged: the merged surface has no triangle (no tet contributes inside the grid)")
            if texture_res is None:
                texture_res = 1024
                while True:
                    try:
                        atlas.atlas_layout(n_tri, texture_res)
                        break
                    except ValueError:
                        texture_res *= 2
                        if texture_res > 32768:
                            raise ValueError(f"MeshRasterizer.export_merged: no texture_res up to 32768 holds the {n_tri} triangles of the "
                                             f"merged surface at grid {grid}; use a coarser grid") from None
            v_tex, t_tex_idx = atlas.atlas_uv(n_tri, texture_res)
            tex = atlas.bake_material(self.materials, merged.v, merged.faces, texture_res)
        atlas.write_textured_obj(out_dir, "merged_surface", merged.v, merged.faces, v_tex, t_tex_idx, tex)
        return merged
