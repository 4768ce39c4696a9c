#!/usr/bin/env python3
"""The reference's texture stage (trainer.py:44-49,56,102-104) on this package: geometry frozen, ExplicitMaterial (hash grid +
VanillaMLP) as the renderer's materials, `L1Loss` on RGB x 20, AdamUniform over renderer.parameters().  The targets are rendered
here from a known colour field on tests/golden/mario_mesh.npz under scenes.dataset_mvps(views) (the reference's img_data/ is
empty).

    python tools/train_texture.py [--views 16 --res 256 --iters 300 --lr 0.01 --mlp VanillaMLP|FullyFusedMLP
                                    --param-grad atomic|sorted --plan-points --shade operators|fused|fused-loss --export DIR]

--plan-points: the views are fixed and the geometry frozen, so the renderer plans them once before the loop
(MeshRasterizer.plan_views) and every iteration runs with view_plan=: no rasterise / interpolate / compaction, and the hash
grid's dL/dparams by the planned route (no sort, no float atomics).

--shade: the image side of an iteration.  `operators` (default): the reference's chain -- antialias of alpha, zero image, masked
scatter, lerp, antialias, slices, L1Loss.  `fused` (MeshRasterizer(fused_shade=True): dr.shade on the view plan's blend plan, then
L1Loss) or `fused-loss` (MeshRasterizer.shade_loss: dr.shade_l1; the only image it writes is the `shaded` it returns); both need --plan-points.  The JSON line
names the mode and, for the fused ones, the blend plan's size ("n_blends", "blend_plan_build_ms", "blend_plan_bytes").

--export DIR: after the fit, renderer.export(DIR, "material") (trainer.py's last step) writes DIR/material/exported_surface.obj,
.mtl and .png; the JSON line gains "export": the bake and the whole export in ms at texture_res = 1024.

One JSON line: the loss at the first and last iteration, ms per iteration, and the split of one iteration's forward + backward
into encode (hash grid), MLP and the rest (rasterise, interpolate, antialias, loss), timed stage by stage on the same points."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Field(torch.nn.Module):
    """The known colour field the targets are rendered from."""

    def forward(self, positions):
        return {"color": 0.5 + 0.5 * torch.sin(torch.stack([3.0 * positions[..., 0] + 1.0, 4.0 * positions[..., 1],
                                                             5.0 * positions[..., 2] - 0.5], -1))}


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def run(views=16, res=256, iters=300, lr=0.01, mlp_otype="VanillaMLP", param_grad="atomic", plan_points=False, export_dir=None, shade="operators"):
    if shade != "operators" and not plan_points:
        raise SystemExit("--shade fused / fused-loss needs --plan-points (the blend plan belongs to a view plan)")
    from tssplat_amd import geometry, materials, renderers, scenes
    from tssplat_amd.utils.optimizer import AdamUniform
    torch.cuda.set_device(0)
    m = np.load(os.path.join(ROOT, "tests", "golden", "mario_mesh.npz"))
    v, f = m["vertices"].astype(np.float32), m["faces"].astype(np.int32)
    geo = geometry.TetMeshGeometry(v, np.zeros((0, 4), np.int32), use_smooth_barrier=False, optimize_geo=False,
                                   surface_vid=np.arange(v.shape[0], dtype=np.int32), surface_fid=f)
    mvp = torch.from_numpy(scenes.dataset_mvps(views).astype(np.float32)).cuda()
    bg = torch.ones(views, res, res, 3, device="cuda")
    with torch.no_grad():
        target = renderers.MeshRasterizer(geo, Field())(mvp, only_alpha=False, iter_num=0, resolution=res, background=bg)["shaded"].clone()
    torch.manual_seed(0)
    cfg = {"n_output_dims": 3, "material_activation": "sigmoid"}
    if mlp_otype != "VanillaMLP":                      # the default config's 32 -> 64 -> 3 network, served by tcnn.Network
        cfg["mlp_network_config"] = {"otype": mlp_otype, "activation": "ReLU", "output_activation": "none", "n_neurons": 64,
                                     "n_hidden_layers": 1}
    if param_grad != "atomic":                         # the encoding's route to dL/dparams, as a key of its config
        cfg["pos_encoding_config"] = dict(materials.ExplicitMaterial.Config(**cfg).pos_encoding_config, param_grad=param_grad)
    mat = materials.ExplicitMaterial(cfg)
    ren = renderers.MeshRasterizer(geo, mat, fused_shade=shade == "fused")
    opt = AdamUniform(ren.parameters(), lr=lr)
    loss_fn = torch.nn.L1Loss()

    view_plan, plan_build_ms = None, None
    if plan_points:
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        view_plan = ren.plan_views(mvp, res)
        b.record()
        torch.cuda.synchronize()
        plan_build_ms = a.elapsed_time(b)
    blend_info = {}
    if shade != "operators":
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        blend_plan = view_plan.blend_plan
        b.record()
        torch.cuda.synchronize()
        blend_info = {"n_blends": blend_plan.n_blends, "blend_plan_build_ms": round(a.elapsed_time(b), 3), "blend_plan_bytes": blend_plan.nbytes}

    def step(it):
        if shade == "fused-loss":
            loss = ren.shade_loss(view_plan, bg, target, it)["img_loss"] * 20
        else:
            out = ren(mvp, only_alpha=False, iter_num=it, resolution=res, background=bg, view_plan=view_plan)
            loss = loss_fn(out["shaded"][..., :3], target[..., :3]) * 20           # trainer.py:102-104
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return loss

    losses = []
    step(0)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for it in range(iters):
        losses.append(step(it).detach())
    b.record()
    torch.cuda.synchronize()
    ms_iter = a.elapsed_time(b) / iters
    losses = [float(l) for l in losses]

    # stage split on the same foreground points
    with torch.no_grad():
        from tssplat_amd import dr
        pos_clip = ren.transform_pos(mvp, geo.tet_v).contiguous()
        rast, _ = dr.rasterize(ren.glctx, pos_clip, geo.surface_fid, resolution=[res, res], grad_db=False)
        p, _ = dr.interpolate(geo.tet_v[None], rast, geo.surface_fid)
        pts = materials.contract_to_unisphere(p[rast[..., 3] > 0], mat.bbox).contiguous()
    enc, mlp = mat.encoding, mat.feature_network
    e = enc(pts).detach()
    ge = torch.randn_like(e)
    gm = torch.randn(pts.shape[0], 3, device="cuda")

    enc_in = mat.encoding.plan_points(pts) if plan_points else pts

    def enc_fb():
        enc(enc_in).backward(ge)

    def mlp_fb():
        mlp(e.requires_grad_(True)).backward(gm)
    ms_enc, ms_mlp = timed(enc_fb), timed(mlp_fb)
    export = {}
    if export_dir is not None:
        import time
        from tssplat_amd import atlas
        texture_res = 1024
        bake_ms = timed(lambda: atlas.bake_material(mat, geo.tet_v[geo.surface_vid.long()], geo.surface_fid, texture_res), reps=3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ren.export(export_dir, "material", texture_res=texture_res)
        torch.cuda.synchronize()
        export = {"export": {"dir": os.path.join(export_dir, "material"), "texture_res": texture_res, "triangles": int(f.shape[0]),
                             "bake_material_ms": round(bake_ms, 3), "export_ms": round((time.perf_counter() - t0) * 1e3, 1)}}
    split_plan = {} if not plan_points else {"plan_build_ms": round(plan_build_ms, 3), "plan_bytes": view_plan.point_plan.nbytes}
    return {"views": views, "res": res, "iters": iters, "lr": lr, "mlp": mlp_otype, "param_grad": "planned" if plan_points else param_grad,
            "shade": shade, **blend_info, "foreground_points": int(pts.shape[0]),
            "loss_first_last": [round(losses[0], 5), round(losses[-1], 5)], "loss_ratio": round(losses[-1] / losses[0], 4),
            "ms_per_iter": round(ms_iter, 3),
            "split_ms": {"encode_fwd_bwd": round(ms_enc, 3), "mlp_fwd_bwd": round(ms_mlp, 3),
                         "render_loss_optimizer_rest": round(ms_iter - ms_enc - ms_mlp, 3), **split_plan}, **export}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--mlp", default="VanillaMLP", help="mlp_network_config otype (VanillaMLP or FullyFusedMLP)")
    ap.add_argument("--param-grad", choices=("atomic", "sorted"), default="atomic",
                    help="the hash grid's route to dL/dparams (sorted: bitwise repeatable)")
    ap.add_argument("--plan-points", action="store_true",
                    help="plan the fixed views once (MeshRasterizer.plan_views) and train with view_plan=")
    ap.add_argument("--shade", choices=("operators", "fused", "fused-loss"), default="operators",
                    help="the image side of an iteration (fused / fused-loss: dr.shade / dr.shade_l1 on the view plan's blend plan; need --plan-points)")
    ap.add_argument("--export", metavar="DIR", default=None,
                    help="after the fit, write DIR/material/exported_surface.{obj,mtl,png} (MeshRasterizer.export)")
    a = ap.parse_args()
    print(json.dumps(run(a.views, a.res, a.iters, a.lr, a.mlp, a.param_grad, a.plan_points, a.export, a.shade)))


if __name__ == "__main__":
    main()
