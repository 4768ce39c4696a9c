#!/usr/bin/env python3
"""BASELINE config 5 on the reference's own object: the geometry-fitting loop of /root/reference/trainer.py:56-134 with the
schedule of config/gso.yaml, fitted to silhouettes of mesh_data/mario_example/model.obj (tests/golden/mario_mesh.npz: the GSO
mesh centred, scaled into the unit ball and decimated -- tests/golden/make_mesh_goldens.py).

What stands in for what the image does not have (img_data/ is empty in the reference, Mitsuba / TetWild / libpgo / omegaconf are
absent):
* the 120 target alpha images are rendered HERE, with tssplat_amd.dr, from the cameras of data/render_dataset.py:15-148
  (`scenes.dataset_mvps`: golden-ratio spiral at radius 4, fov 39.3, the script's look_at and perspective);
* the tet-spheres are kuhn balls (no TetWild) placed greedily in the visual hull of those images -- largest inscribed ball of
  the still-uncovered part first -- instead of the reference's offline key-point file (geometry.key_points_file_path, a MILP
  coverage solution; tetmesh_geometry.py:268-290 only scales and moves the template sphere to each key point);
* everything else is the reference's loop: `img_loss = MSE(alpha) * 20`, `loss = img_loss * 100 + reg`, `AdamUniform(lr 0.2,
  grad_limit 0.01)`, cosine schedule, order 2 -> 4 at iteration 1 000, smooth_eng_coeff / n_spheres (tetmesh_geometry.py:242).

    python tools/train_object.py [--spheres 20 --k 8 --views 120 --res 512 --iters 1500 --silhouette operators|fused|fused-loss --no-stages]
                                 [--fit-depth off|operators|fused-loss --fit-depth-start N] [--depth-bench PATH]
                                 [--fit-normal off|operators|fused-loss --fit-normal-start N --normal-weight W] [--normal-bench PATH]
                                 [--placement host|device|mesh --grid N] [--merge-grid N --merge-out DIR --merge-fill none|cavities|outer --merge-simplify K] [--eval-samples N [--eval-exact]] [--eval-grid N] [--eval-quality]

--placement: where the tet-spheres are placed -- `host` (the default, `place_spheres` + `build_spheres` below: torch, scipy and numpy,
so that recorded runs stay comparable) or `device` (`tssplat_amd.spheres_init.init_spheres` + `geometry.TetMeshMultiSphereGeometry`:
the same algorithm as HIP kernels, stated in integers) or `mesh` (the same cover, `spheres_init.cover_occupancy`, of the target mesh's own
occupancy, `tssplat_amd.voxelize.occupancy` on the cube (-1, 1), instead of the silhouettes' visual hull).  --grid: voxels per axis of the placement grid (72).

--silhouette: how the loop renders alpha and takes the image loss -- `operators` (the default: rasterize, clamp, antialias, MSELoss),
`fused` (MeshRasterizer(fused_silhouette=True): dr.silhouette, then MSELoss) or `fused-loss` (MeshRasterizer.silhouette_loss:
dr.silhouette_mse, no gradient image).  --no-stages: leave out the stand-alone stage timings (`stages_ms`).

--fit-depth: the trainer's depth term (trainer.py:77-79, :106-109: `+ MSE(d * a_ref, d_ref * a_ref) * 100` once `it` has passed
--fit-depth-start) -- `operators` (forward(fit_depth=True): rasterize, antialias, interpolate, norm, two MSELoss calls) or
`fused-loss` (MeshRasterizer.silhouette_depth_loss: one rasterisation, no image chain); before the start the loop is --silhouette's.
The target distances are rendered once, without gradients, from the target mesh by the operator chain.  --depth-bench PATH: both
modes on the same seed plus the depth stage timings (median of five repeats of 200 iterations, HIP events), written to PATH
(profiles/depth_bench.json).

--fit-normal: a normal term, `+ MSE(n * a_ref, n_ref * a_ref) * --normal-weight` once `it` has passed --fit-normal-start, with
`n = out["n"]` of mesh_rasterizer.py:137-149 (the interpolated vertex normals times [1, 1, -1]).  The reference's renderer returns
that image and its dataset loads normal maps, but its trainer has no normal line: the default weight 100 mirrors the depth term's
`* 100`.  `operators`: forward(fit_normal=True) and a masked MSELoss; `fused-loss`: MeshRasterizer.silhouette_normal_loss.  With
--fit-depth in the same mode the three terms come from one forward -- under `fused-loss` from one rasterisation; the two options must
name the same mode when both are on.  The target normals are rendered once, without gradients, from the target mesh by the operator
chain with the same [1, 1, -1] convention.  --normal-bench PATH: --fit-normal alone and with --fit-depth, each in both modes on the same
seed, plus the normal stage timings (median of five windows of 200 calls, HIP events), written to PATH (profiles/normal_bench.json).

--merge-grid N: after the fit, `tssplat_amd.merge` (`union_field`, `extract_surface`: what `merge_tets` runs) turns all spheres into ONE closed surface at N nodes per axis
(`merged_surface.obj` under --merge-out) and the record gains `merged`: `closed`, the counts and `volume_iou_vs_hull`, the merged
solid's occupancy against `spheres_init.visual_hull` of the target silhouettes at the same grid and bounds.
--merge-fill none|cavities|outer: `merge.fill_field` between the field and the extraction; `merged` then also holds `cavities`,
`cavity_nodes`, `islands`, `island_nodes`, the Euler characteristic V - F / 2 and the triangle count before (`unfilled`) and after.
--merge-simplify K (0: off; an integer >= 2): `tssplat_amd.simplify.simplify` clusters the extracted (and filled) surface on N // K cells per axis of the merge's
bounds; `merged_surface.obj` is then the clustered mesh and `merged` gains `simplify`: the counts before and after, `edge_stats`, and with --eval-samples
`vs_unsimplified` (`metrics.compare_meshes(simplified, unsimplified)`) next to `eval`'s `merged_simplified` against the target mesh.

--merge-smooth N (0: off): `tssplat_amd.smooth.smooth` runs N iterations on the surface handed out (after the fill and the simplification), once per mode; `merged`
gains `smooth`: per mode who moved and who was held and, with --eval-quality, `quality.shape`'s figures, the crossing pairs and `watertight` before and after, with
--eval-samples --eval-exact `vs_unsmoothed_exact` (`metrics.compare_meshes_exact(smoothed, unsmoothed)`), and `merged_smoothed_<mode>` in `eval`, `eval_exact`,
`eval_quality` and `volume_iou_vs_target`.  `merged_surface.obj` holds the default mode's vertices.  Faces and `closed` are untouched; crossing pairs are reported as found.

--eval-samples N (0: off, the record is what it was): `eval`, `tssplat_amd.metrics.compare_meshes` on N samples per surface against the TARGET MESH --
Chamfer distance, accuracy / completeness, F-score, normal consistency, each with its `noise_floor` -- of `raw_union` (the concatenated tet-sphere
boundaries, interior sheets included), `merged` (with --merge-grid) and `merged_filled` (with --merge-fill).
--eval-quality: `eval_quality`, the record of `tssplat_amd.quality.mesh_quality` (crossing pairs on a 2^20 lattice, edge / vertex manifoldness, components,
orientation, Euler characteristic, area-length ratio and minimum angle) for `raw_union`, `target` and whichever of `merged`, `merged_filled`, `merged_simplified` the run makes.
--eval-exact (with --eval-samples): `eval_exact` next to `eval`, the same surfaces through `tssplat_amd.metrics.compare_meshes_exact` -- samples against the triangles
themselves, so the figures have no sampling floor (`noise_floor` is then a rounding-level number) -- and `vs_unsimplified_exact` next to `vs_unsimplified`.

--eval-grid N (0: off, the record is what it was): `volume_iou_vs_target`, `tssplat_amd.voxelize.mesh_volume_iou` at N nodes per axis against the TARGET MESH (winding
number, rule "nonzero", three rays, bounds spanning both meshes) of `raw_union`, `merged`, `merged_filled` and `merged_simplified`, each with its inside counts, open
columns and disputed nodes; for `merged` and `merged_filled` also `on_merge_grid`: the surface voxelised on the merge's own grid and bounds, and the number of nodes
at which that differs from `merge.occupancy` of the field it was extracted from.

One JSON line: silhouette IoU over all views, inverted tets, seconds per iteration and the stand-alone stage times."""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def render_alpha(glctx, verts, tri, mvp, res):
    """Antialiased alpha image of a triangle mesh: the alpha branch of MeshRasterizer.forward (mesh_rasterizer.py:101-108)."""
    import torch
    import tssplat_amd.dr as dr
    posw = torch.cat([verts, torch.ones_like(verts[:, :1])], dim=1)
    pos_clip = torch.matmul(posw, mvp.transpose(1, 2)).contiguous()
    rast, _ = dr.rasterize(glctx, pos_clip, tri, resolution=[res, res], grad_db=False)
    alpha = torch.clamp(rast[..., -1:], 0, 1).contiguous()
    return dr.antialias(alpha, rast, pos_clip, tri)


def render_depth(glctx, verts, tri, mvp, campos, res):
    """Distance-to-camera image of a triangle mesh, `[B, H, W, 1]`: the depth branch of MeshRasterizer.forward (mesh_rasterizer.py:150-161)."""
    import torch
    import tssplat_amd.dr as dr
    posw = torch.cat([verts, torch.ones_like(verts[:, :1])], dim=1)
    pos_clip = torch.matmul(posw, mvp.transpose(1, 2)).contiguous()
    rast, _ = dr.rasterize(glctx, pos_clip, tri, resolution=[res, res], grad_db=False)
    world, _ = dr.interpolate(verts[None, ...].contiguous(), rast, tri)
    return torch.norm(world - campos[:, None, None, :], dim=-1, keepdim=True)


def vertex_normals(verts, tri):
    """Unit vertex normals of a triangle mesh in plain torch (this runs once, for the target): every triangle adds its area-weighted
    normal to its three corners; a vertex whose sum vanishes gets +z."""
    import torch
    t = tri.long()
    corners = verts[t]                                                                   # [T, 3 corners, 3]
    face = torch.linalg.cross(corners[:, 1] - corners[:, 0], corners[:, 2] - corners[:, 0])
    total = torch.zeros_like(verts).index_add_(0, t.reshape(-1), face.repeat_interleave(3, dim=0))
    flat = (total * total).sum(dim=1, keepdim=True) <= 1e-20
    total = torch.where(flat, total.new_tensor([0.0, 0.0, 1.0]), total)
    return total / total.norm(dim=1, keepdim=True)


def render_normal(glctx, verts, tri, mvp, res):
    """Normal image of a triangle mesh, `[B, H, W, 3]`: the normal branch of MeshRasterizer.forward (mesh_rasterizer.py:137-149), the
    vertex normals times [1, 1, -1] interpolated, 0 on background."""
    import torch
    import tssplat_amd.dr as dr
    posw = torch.cat([verts, torch.ones_like(verts[:, :1])], dim=1)
    pos_clip = torch.matmul(posw, mvp.transpose(1, 2)).contiguous()
    rast, _ = dr.rasterize(glctx, pos_clip, tri, resolution=[res, res], grad_db=False)
    attr = vertex_normals(verts, tri) * verts.new_tensor([1.0, 1.0, -1.0])
    return dr.interpolate(attr[None, ...].contiguous(), rast, tri)[0]


def place_spheres(target_alpha, mvp, n_spheres, grid=72, min_radius=0.05, shrink=0.92):
    """Greedy ball placement in the visual hull of the target silhouettes.  A voxel of [-1, 1]^3 is inside when every view sees
    it on the object; the Euclidean distance transform of the hull gives each voxel's largest inscribed ball; pick the largest
    ball whose CENTRE is not yet covered, mark what it covers, repeat."""
    import numpy as np
    import torch
    from scipy import ndimage
    B, H, W = target_alpha.shape[:3]
    lin = (np.arange(grid) + 0.5) / grid * 2 - 1
    P = np.stack(np.meshgrid(lin, lin, lin, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    pts = torch.from_numpy(np.concatenate([P, np.ones((P.shape[0], 1), np.float32)], axis=1)).to(mvp.device)
    inside = torch.ones(P.shape[0], dtype=torch.bool, device=mvp.device)
    occ = target_alpha[..., 0] > 0.5
    for b in range(B):
        clip = pts @ mvp[b].T
        ndc = clip[:, :2] / clip[:, 3:4]
        px = ((ndc[:, 0] + 1) * 0.5 * W).floor().long().clamp(0, W - 1)
        py = ((ndc[:, 1] + 1) * 0.5 * H).floor().long().clamp(0, H - 1)       # row 0 = bottom, like the rasteriser's output
        inside &= occ[b, py, px] & (ndc.abs() < 1).all(dim=1)
    hull = inside.reshape(grid, grid, grid).cpu().numpy()
    h = 2.0 / grid
    dist = ndimage.distance_transform_edt(hull) * h
    uncovered = hull.copy()
    centres, radii = [], []
    for _ in range(n_spheres):
        score = np.where(uncovered, dist, 0.0)
        k = int(np.argmax(score))
        r = float(score.flat[k]) * shrink
        if r < min_radius:
            break
        c = P[k]
        centres.append(c)
        radii.append(r)
        uncovered &= (np.linalg.norm(P - c, axis=1) > r).reshape(hull.shape)
    return np.asarray(centres, np.float32), np.asarray(radii, np.float32), float(hull.mean()), float(uncovered.sum()) / max(1.0, float(hull.sum()))


def build_spheres(centres, radii, k):
    """`kuhn_ball(k)` scaled and moved to every (centre, radius): the concatenation of tetmesh_geometry.py:310-331."""
    import numpy as np
    from tssplat_amd import scenes
    bv, bt = scenes.kuhn_ball(k)
    bv = bv / np.linalg.norm(bv, axis=1).max()
    rest, tets = [], []
    for s, (c, r) in enumerate(zip(centres, radii)):
        rest.append((bv * r + c).astype(np.float32))
        tets.append(bt + s * bv.shape[0])
    return np.concatenate(rest), np.concatenate(tets).astype(np.int32)


def surface_topology(field, level, n_vertices, n_triangles):
    """What the extraction of a closed `field` consists of, from `merge.components`: the inside and outside components of its nodes,
    the closed surfaces between them (inside + outside - 1: their adjacency is a tree), the Euler characteristic V - F / 2 and the
    handles it leaves, surfaces - chi / 2 (a closed surface of genus g has chi = 2 - 2 g)."""
    import torch
    from tssplat_amd import merge
    label = merge.components(field, level).reshape(-1)
    root = label == torch.arange(label.numel(), dtype=torch.int32, device=label.device)
    inside = merge.occupancy(field, level).reshape(-1)
    n_in, n_out = (int(x) for x in torch.stack([(root & inside).sum(), (root & ~inside).sum()]).cpu().numpy())
    chi = int(n_vertices) - int(n_triangles) // 2
    surfaces = n_in + n_out - 1
    return {"inside_components": n_in, "outside_components": n_out, "surfaces": surfaces, "euler_characteristic": chi, "handles": surfaces - chi // 2}


def run(target_npz=None, n_spheres=20, k=8, views=120, res=512, iters=1500, log_every=100, stages=True, verbose=False, silhouette="operators",
        fit_depth="off", fit_depth_start=0, depth_stage_reps=(20, 1), fit_normal="off", fit_normal_start=0, normal_weight=100.0, normal_stage_reps=(20, 1), placement="host", grid=72, merge_grid=0, merge_out=None,
        merge_fill="none", eval_samples=0, merge_simplify=0, eval_grid=0, eval_exact=False, eval_quality=False, merge_smooth=0):
    import numpy as np
    import torch
    import tssplat_amd.dr as dr
    from tssplat_amd import geometry, renderers, scenes
    from tssplat_amd.utils.optimizer import AdamUniform

    if silhouette not in ("operators", "fused", "fused-loss"):
        raise ValueError(f"unknown --silhouette mode {silhouette!r}")
    if fit_depth not in ("off", "operators", "fused-loss"):
        raise ValueError(f"unknown --fit-depth mode {fit_depth!r}")
    if fit_normal not in ("off", "operators", "fused-loss"):
        raise ValueError(f"unknown --fit-normal mode {fit_normal!r}")
    if "off" not in (fit_normal, fit_depth) and fit_normal != fit_depth:
        raise ValueError(f"--fit-normal {fit_normal} with --fit-depth {fit_depth}: the two terms share one forward, so they must name the same mode")
    if placement not in ("host", "device", "mesh"):
        raise ValueError(f"unknown --placement {placement!r}")
    target_npz = target_npz or os.path.join(ROOT, "tests", "golden", "mario_mesh.npz")
    tgt = np.load(target_npz)
    tv = torch.from_numpy(tgt["vertices"].astype(np.float32)).cuda()
    tf = torch.from_numpy(tgt["faces"].astype(np.int32)).cuda()
    mvp = torch.from_numpy(scenes.dataset_mvps(views)).cuda()
    glctx = dr.RasterizeCudaContext()
    with torch.no_grad():
        target = render_alpha(glctx, tv, tf, mvp, res).clone()
    campos = torch.from_numpy(scenes.dataset_campos(views)).cuda()
    if fit_depth != "off":
        with torch.no_grad():
            target_depth = render_depth(glctx, tv, tf, mvp, campos, res).clone()
    if fit_normal != "off":
        with torch.no_grad():
            target_normal = render_normal(glctx, tv, tf, mvp, res).clone()
    if placement in ("device", "mesh"):
        from tssplat_amd import spheres_init
        if placement == "mesh":    # the target mesh is at hand: cover its own occupancy, not the visual hull of its silhouettes
            from tssplat_amd import voxelize
            kp = spheres_init.cover_occupancy(voxelize.occupancy(tv, tf, grid, (-1.0, 1.0)).occ, n_spheres, (-1.0, 1.0))
        else:
            kp = spheres_init.init_spheres(target, mvp, n_spheres, grid=grid)
        radii, hull_frac, left, S = kp.r, kp.hull_fraction, kp.uncovered_fraction, len(kp)
        flags = types.SimpleNamespace(smooth_eng_coeff=2e-4, barrier_coeff=2e-4, increase_order_iter=1000)   # gso.yaml:8-11; the class divides by S
        geo = geometry.TetMeshMultiSphereGeometry(kp, k=k, smooth_barrier_param=flags)
        rest, tets = geo.tet_v.detach().cpu().numpy(), geo.tet_elem.cpu().numpy()
    else:
        centres, radii, hull_frac, left = place_spheres(target, mvp, n_spheres, grid=grid)
        S = len(radii)
        rest, tets = build_spheres(centres, radii, k)
        flags = types.SimpleNamespace(smooth_eng_coeff=2e-4 / S, barrier_coeff=2e-4, increase_order_iter=1000)   # gso.yaml:8-11, tetmesh_geometry.py:242-243
        geo = geometry.TetMeshGeometry(rest, tets, smooth_barrier_param=flags)
    ren = renderers.MeshRasterizer(geo, fused_silhouette=silhouette != "operators")
    opt = AdamUniform(ren.parameters(), lr=0.2, grad_limit=True, grad_limit_values=[0.01, 0.01], grad_limit_iters=[1500])   # gso.yaml:37-41
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, iters, eta_min=1e-4)                                           # trainer.py:57-58
    shade_loss = torch.nn.MSELoss()
    log = []

    def iou_now(it):
        with torch.no_grad():
            final = ren(mvp, only_alpha=True, iter_num=it, resolution=res)["shaded"]
            a, b = final[..., -1] > 0.5, target[..., -1] > 0.5
            return float((a & b).sum()) / max(1.0, float((a | b).sum()))

    iou0 = iou_now(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for it in range(iters):
        depth_on = fit_depth != "off" and fit_depth_start < it
        if fit_normal == "fused-loss" and fit_normal_start < it:
            depth_args = {"campos": campos, "target_depth": target_depth} if depth_on else {}
            out = ren.silhouette_normal_loss(mvp, target, target_normal, iter_num=it, resolution=res, **depth_args)
            img_loss = out["img_loss"] * 20 + out["normal_loss"] * normal_weight
            if depth_on:
                img_loss = img_loss + out["depth_loss"] * 100
        elif fit_normal == "operators" and fit_normal_start < it:
            out = ren(mvp, only_alpha=True, iter_num=it, resolution=res, fit_normal=True, fit_depth=depth_on, campos=campos)
            img_loss = shade_loss(out["shaded"][..., -1], target[..., -1]) * 20
            img_loss = img_loss + shade_loss(out["n"] * target, target_normal * target) * normal_weight
            if depth_on:
                img_loss = img_loss + shade_loss(out["d"][..., -1] * target[..., -1], target_depth[..., -1] * target[..., -1]) * 100
        elif fit_depth == "fused-loss" and fit_depth_start < it:
            out = ren.silhouette_depth_loss(mvp, target, campos, target_depth, iter_num=it, resolution=res)
            img_loss = out["img_loss"] * 20 + out["depth_loss"] * 100
        elif fit_depth == "operators" and fit_depth_start < it:                          # trainer.py:77-79, :106-109
            out = ren(mvp, only_alpha=True, iter_num=it, resolution=res, fit_depth=True, campos=campos)
            img_loss = shade_loss(out["shaded"][..., -1], target[..., -1]) * 20
            img_loss = img_loss + shade_loss(out["d"][..., -1] * target[..., -1], target_depth[..., -1] * target[..., -1]) * 100
        elif silhouette == "fused-loss":
            out = ren.silhouette_loss(mvp, target, iter_num=it, resolution=res)
            img_loss = out["img_loss"] * 20
        else:
            out = ren(mvp, only_alpha=True, iter_num=it, resolution=res)
            img_loss = shade_loss(out["shaded"][..., -1], target[..., -1]) * 20        # trainer.py:99-101
        loss = img_loss * 100 + out["geo_regularization"]                              # trainer.py:115
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        sched.step()
        if it % log_every == 0 or it == iters - 1:
            log.append((it, float(img_loss.detach()), float(out["geo_regularization"].detach())))
            if verbose:
                print(log[-1], file=sys.stderr)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    iou = iou_now(iters)
    x = geo.tet_v.detach().cpu().numpy().astype(np.float64)

    def dets(p):
        return np.linalg.det(np.stack([p[tets[:, 1]] - p[tets[:, 0]], p[tets[:, 2]] - p[tets[:, 0]], p[tets[:, 3]] - p[tets[:, 0]]], axis=1))
    inverted = int((np.sign(dets(x)) != np.sign(dets(rest.astype(np.float64)))).sum())
    rec = {
        "metric": "s per iteration, geometry-fitting loop on the reference's object (BASELINE config 5)", "value": dt / iters, "unit": "s/iteration",
        "higher_is_better": False, "silhouette": silhouette, "fit_depth": fit_depth, "fit_depth_start": fit_depth_start,
        "fit_normal": fit_normal, "fit_normal_start": fit_normal_start, "normal_weight": normal_weight, "iterations": iters, "wall_s": dt, "ms_per_iteration": 1e3 * dt / iters,
        "silhouette_iou": iou, "silhouette_iou_at_start": iou0, "inverted_tets": inverted, "tets": int(tets.shape[0]),
        "img_loss_first_last": [log[0][1], log[-1][1]], "reg_first_last": [log[0][2], log[-1][2]],
        "spheres": {"placed": S, "asked": n_spheres, "radii_min_max": [float(radii.min()), float(radii.max())], "visual_hull_fraction_of_cube": hull_frac,
                    "hull_voxel_centres_left_uncovered": left, "placement": placement, "grid": grid},
        "config": {"workload": f"{S} tet-spheres x kuhn{k}: {int(tets.shape[0])} tets, {int(geo.surface_fid.shape[0])} surface triangles; {views} views x {res}^2 per iteration; "
                               f"target {os.path.basename(target_npz)} ({int(tv.shape[0])} vertices, {int(tf.shape[0])} triangles)",
                   "data": "silhouettes of the reference's mesh_data/mario_example/model.obj rendered with tssplat_amd.dr from data/render_dataset.py's cameras",
                   "schedule": "config/gso.yaml: lr 0.2 cosine, grad_limit 0.01, order 2 -> 4 at 1000, coeff_scheduler, smooth_eng_coeff / n_spheres"},
        "log": log,
    }
    evals, exacts = {}, {}

    def evaluate(key, v, f):   # 3-D figures against the target mesh itself: Chamfer distance, F-score, normal consistency and their noise floor
        from tssplat_amd import metrics
        evals[key] = {"triangles": int(f.shape[0]), **metrics.compare_meshes(v.contiguous(), f.contiguous(), tv, tf, n=eval_samples, seed=0).as_dict()}
        if eval_exact:         # the same samples against the triangles themselves: no sampling floor
            exacts[key] = {"triangles": int(f.shape[0]), **metrics.compare_meshes_exact(v.contiguous(), f.contiguous(), tv, tf, n=eval_samples, seed=0).as_dict()}
    if eval_samples:           # (a) the raw concatenated tet-sphere boundary surface: interior sheets wherever spheres overlap
        evaluate("raw_union", geo.tet_v.detach()[geo.surface_vid.long()], geo.surface_fid)
    quals = {}

    def grade(key, v, f):      # what kind of mesh it is: crossing pairs on the 2^20 lattice, topology, triangle shape (tssplat_amd.quality)
        from tssplat_amd import quality
        quals[key] = {"triangles": int(f.shape[0]), **quality.mesh_quality(v.contiguous(), f.contiguous()).as_dict()}
    if eval_quality:
        grade("raw_union", geo.tet_v.detach()[geo.surface_vid.long()], geo.surface_fid)
        grade("target", tv, tf)
    vols = {}

    def volume(key, v, f, field=None, grid_bounds_level=None):   # volume IoU against the target mesh: both voxelised (winding number, rule "nonzero", three rays)
        from tssplat_amd import merge, voxelize
        r = voxelize.mesh_volume_iou(v.contiguous(), f.contiguous(), tv, tf, grid=eval_grid)
        vols[key] = {"iou": r["iou"], "inside": r["inside_a"], "inside_target": r["inside_b"], "bounds": list(r["bounds"]), "open_columns": list(r["a"].open_columns),
                     "disputed": r["a"].disputed, "target_open_columns": list(r["b"].open_columns), "target_disputed": r["b"].disputed}
        if field is not None:      # ... and, on the merge's own grid, the voxelised surface against the occupancy of the field it was extracted from
            g, b, lv = grid_bounds_level
            own = voxelize.occupancy(v.contiguous(), f.contiguous(), g, b)
            vols[key]["on_merge_grid"] = {"nodes_differing_from_merge_occupancy": int((own.occ != merge.occupancy(field, lv)).sum()), "inside": int(own.occ.sum()),
                                          "open_columns": list(own.open_columns), "disputed": own.disputed}
    if eval_grid:
        volume("raw_union", geo.tet_v.detach()[geo.surface_vid.long()], geo.surface_fid)
    if merge_grid:  # the fitted spheres as ONE closed surface, and a 3-D figure: its occupancy against the targets' visual hull
        from tssplat_amd import merge, spheres_init
        tet_v = geo.tet_v.detach()
        bounds = merge.default_bounds(tet_v, merge_grid)
        level = merge.default_level(merge_grid, bounds)
        field = merge.union_field(tet_v, geo.tet_elem, merge_grid, bounds)
        mv, mf, closed = merge.extract_surface(field, bounds, level)
        if eval_samples:       # (b) the merged surface
            evaluate("merged", mv, mf)
        if eval_quality:
            grade("merged", mv, mf)
        if eval_grid:
            volume("merged", mv, mf, field, (merge_grid, bounds, level))
        fill_rec = {"fill": merge_fill}
        if merge_fill != "none":   # the flood fill: what it removed, in components, nodes, triangles and Euler characteristic (V - F / 2 on a closed mesh)
            filled = merge.fill_field(field, level, merge_fill)
            before = {"vertices": int(mv.shape[0]), "triangles": int(mf.shape[0]), **surface_topology(field, level, mv.shape[0], mf.shape[0])}
            field = filled.field
            mv, mf, closed = merge.extract_surface(field, bounds, level)
            if eval_samples:   # (c) the filled merged surface
                evaluate("merged_filled", mv, mf)
            if eval_quality:
                grade("merged_filled", mv, mf)
            if eval_grid:
                volume("merged_filled", mv, mf, field, (merge_grid, bounds, level))
            fill_rec.update(cavities=filled.cavities, cavity_nodes=filled.cavity_nodes, islands=filled.islands, island_nodes=filled.island_nodes,
                            unfilled=before, triangles_before=before["triangles"], triangles_after=int(mf.shape[0]))
        fill_rec.update(surface_topology(field, level, mv.shape[0], mf.shape[0]))
        occ = merge.occupancy(field, level)
        if merge_simplify:     # vertex clustering of the surface extracted above on merge_grid // merge_simplify cells of the same cube
            import dataclasses
            from tssplat_amd import metrics, simplify
            k = merge._check_simplify("merge_tets", merge_simplify, merge_grid)
            simp = simplify.simplify(mv, mf, merge_grid // k, bounds)
            fill_rec["simplify"] = {"factor": k, "cells": simp.cells, "placement": simp.placement, "vertices_before": int(mv.shape[0]), "triangles_before": int(mf.shape[0]),
                                    "vertices_after": int(simp.v.shape[0]), "triangles_after": int(simp.faces.shape[0]), "cells_occupied": simp.cells_occupied,
                                    "clamped": simp.clamped, "duplicates": simp.duplicates, "degenerate_faces": simp.degenerate_faces,
                                    "invalid_faces": simp.invalid_faces, "edge_stats": dataclasses.asdict(simplify.edge_stats(simp.faces))}
            if eval_samples:   # (d) the simplified surface: against the unsimplified one, and against the target like the others
                fill_rec["simplify"]["vs_unsimplified"] = metrics.compare_meshes(simp.v, simp.faces, mv.contiguous(), mf.contiguous(), n=eval_samples, seed=0).as_dict()
                if eval_exact:
                    fill_rec["simplify"]["vs_unsimplified_exact"] = metrics.compare_meshes_exact(simp.v, simp.faces, mv.contiguous(), mf.contiguous(), n=eval_samples,
                                                                                                 seed=0).as_dict()
                evaluate("merged_simplified", simp.v, simp.faces)
            if eval_grid:
                volume("merged_simplified", simp.v, simp.faces)
            if eval_quality:
                grade("merged_simplified", simp.v, simp.faces)
            mv, mf, closed = simp.v, simp.faces, simplify.edge_stats(simp.faces).closed
        if merge_smooth:       # tssplat_amd.smooth on the surface handed out: both modes are recorded, the file holds the default mode's vertices; faces and closed stay
            from tssplat_amd import metrics, quality, smooth
            mv, mf = mv.contiguous(), mf.contiguous()
            adj = smooth.adjacency(mf, int(mv.shape[0]))
            fill_rec["smooth"] = {"iterations": merge_smooth, "vertices": int(mv.shape[0]), "triangles": int(mf.shape[0]),
                                  "promise": "faces are untouched; a result free of crossing pairs is reported, not promised"}
            before = quality.mesh_quality(mv, mf) if eval_quality else None
            outs = {}
            for mode in smooth.MODES:
                sm = smooth.smooth(mv, mf, iterations=merge_smooth, mode=mode, adjacency=adj)
                outs[mode] = sm.v
                r = {"lam": sm.lam, "mu": sm.mu, "boundary": sm.boundary, "moved": sm.moved, "held_other": sm.held_other, "held_pinned": sm.held_pinned,
                     "held_irregular": sm.held_irregular}
                if eval_quality:
                    after = quality.mesh_quality(sm.v, mf)
                    for key, q in (("before", before), ("after", after)):
                        r[key] = {"alr_mean": q.shape.alr_mean, "alr_p05": q.shape.alr_p05, "alr_min": q.shape.alr_min, "min_angle_min": q.shape.min_angle_min,
                                  "min_angle_mean": q.shape.min_angle_mean, "crossing_pairs": q.intersections.crossing_pairs, "watertight": q.watertight}
                    grade("merged_smoothed_" + mode, sm.v, mf)
                if eval_samples:
                    if eval_exact:
                        r["vs_unsmoothed_exact"] = metrics.compare_meshes_exact(sm.v, mf, mv, mf, n=eval_samples, seed=0).as_dict()
                    evaluate("merged_smoothed_" + mode, sm.v, mf)
                if eval_grid:
                    volume("merged_smoothed_" + mode, sm.v, mf)
                fill_rec["smooth"][mode] = r
            mv = outs[smooth.DEFAULT_MODE]
        merge_out = merge_out or os.path.join(ROOT, "bench_outputs", "train_object")
        os.makedirs(merge_out, exist_ok=True)
        merge.write_obj(os.path.join(merge_out, "merged_surface.obj"), mv, mf)
        hull = spheres_init.visual_hull(target, mvp, grid=merge_grid, bounds=bounds)
        rec["merged"] = {"file": "merged_surface.obj", "grid": merge_grid, "bounds": list(bounds), "level": level,
                         "vertices": int(mv.shape[0]), "triangles": int(mf.shape[0]), "closed": closed,
                         "inside_fraction": int(occ.sum()) / float(merge_grid ** 3), "volume_iou_vs_hull": merge.volume_iou(occ, hull), **fill_rec}
    if eval_grid:
        rec["volume_iou_vs_target"] = {"grid": eval_grid, "rule": "nonzero", "rays": 3, "reference": os.path.basename(target_npz), **vols}
    if eval_quality:
        rec["eval_quality"] = {"lattice": "2^20 per axis over each surface's own min / max cube", "order": "the default of tssplat_amd.quality", **quals}
    if eval_samples:
        rec["eval"] = {"samples": eval_samples, "seed": 0, "reference": os.path.basename(target_npz), "a": "the surface named by the key", "b": "the target mesh", **evals}
        if eval_exact:
            rec["eval_exact"] = {"samples": eval_samples, "seed": 0, "reference": os.path.basename(target_npz), "a": "the surface named by the key", "b": "the target mesh",
                                 "distances": "samples against triangles (metrics.compare_meshes_exact)", **exacts}
    if stages:      # the stages on their own (HIP events; they overlap nothing, so their sum is close to one iteration)
        def timed(fn, reps=20):
            for j in range(3):
                fn(j)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for j in range(reps):
                fn(3 + j)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / reps

        def timed_alternating(fns, reps, repeats):
            """ms per call of every function of `fns`: `repeats` windows of `reps` calls each, the functions taking turns window by
            window (what shares the machine hits both alike) -> {name: sorted list of the windows' means}"""
            windows = {name: [] for name in fns}
            for _ in range(repeats):
                for name, fn in fns.items():
                    windows[name].append(timed(fn, reps))
            return {name: sorted(t) for name, t in windows.items()}
        data = geo(iter_num=5)
        pos = ren.transform_pos(mvp, data.v_pos).contiguous().detach()
        tri = data.t_pos_idx
        rast, _ = dr.rasterize(ren.glctx, pos, tri, resolution=[res, res], grad_db=False)
        alpha = torch.clamp(rast[..., -1:], 0, 1).contiguous()
        pos_g = pos.clone().requires_grad_(True)
        ga = torch.randn_like(alpha)

        def geo_fb(j):
            geo.tet_v.grad = None
            d = geo(iter_num=j)
            (d.smooth_barrier_energy + d.v_pos.sum() * 0).backward()

        def aa_fb(j):
            pos_g.grad = None
            dr.antialias(alpha, rast, pos_g, tri).backward(ga)

        def sil_fb(j):
            pos_g.grad = None
            dr.silhouette(ren.glctx, pos_g, tri, [res, res]).backward(ga)

        def sil_mse_fb(j):
            pos_g.grad = None
            dr.silhouette_mse(ren.glctx, pos_g, tri, [res, res], target).backward()
        depth_stages = {}
        if fit_depth != "off" and fit_normal == "off":             # (with the normal term on, the stage timings below are that term's)
            # the depth term on its own, forward + backward, given the rasterisation each path starts from: `rast` (kept in the
            # graph: the backward runs interpolate's and rasterize's) against the ids of the alpha stage
            world_g = data.v_pos.detach().clone().requires_grad_(True)
            a_ref, d_ref = target[..., -1].contiguous(), target_depth[..., -1].contiguous()
            rast_g, _ = dr.rasterize(ren.glctx, pos_g, tri, resolution=[res, res], grad_db=False)
            topo = dr.antialias_construct_topology_hash(tri)
            _, ids, _ = dr._silhouette_forward(pos, tri, topo.opp, ren.glctx, res, res)
            lib, check, stream = dr._lib, dr._capi.check, dr._stream_ptr(pos.device)
            B, V, T = int(pos.shape[0]), int(pos.shape[1]), int(tri.shape[0])
            ws = torch.empty(int(lib.tsamd_depth_mse_workspace_bytes(B * res * res)), dtype=torch.uint8, device=pos.device)
            loss_f, one = torch.empty((), device=pos.device), torch.ones((), device=pos.device)
            gw, gp = torch.empty_like(world_g), torch.empty_like(pos)

            def depth_chain_fb(j):
                pos_g.grad = world_g.grad = None
                x, _ = dr.interpolate(world_g[None, ...], rast_g, tri)
                d = torch.norm(x - campos[:, None, None, :], dim=-1, keepdim=True)
                shade_loss(d[..., -1] * a_ref, d_ref * a_ref).backward(retain_graph=True)

            def depth_fused_fb(j):
                args = (pos.data_ptr(), B, V, tri.data_ptr(), T, res, res, ids.data_ptr(), world_g.data_ptr(), campos.data_ptr(), d_ref.data_ptr(), a_ref.data_ptr())
                check(lib.tsamd_depth_mse(*args, ws.data_ptr(), loss_f.data_ptr(), None, stream))
                check(lib.tsamd_depth_mse_backward(*args, one.data_ptr(), 0, gw.data_ptr(), gp.data_ptr(), stream))

            def terms_chain_fb(j):
                pos_g.grad = world_g.grad = None
                r, _ = dr.rasterize(ren.glctx, pos_g, tri, resolution=[res, res], grad_db=False)
                a = dr.antialias(torch.clamp(r[..., -1:].detach(), 0, 1).contiguous(), r, pos_g, tri)
                x, _ = dr.interpolate(world_g[None, ...], r, tri)
                d = torch.norm(x - campos[:, None, None, :], dim=-1, keepdim=True)
                (shade_loss(a[..., -1], a_ref) * 20 + shade_loss(d[..., -1] * a_ref, d_ref * a_ref) * 100).backward()

            def terms_fused_fb(j):
                pos_g.grad = world_g.grad = None
                la, ld = dr.silhouette_depth_mse(ren.glctx, pos_g, tri, [res, res], target, world_g, campos, target_depth, target)
                (la * 20 + ld * 100).backward()
            reps, repeats = depth_stage_reps
            windows = timed_alternating({"depth_operators_forward_backward": depth_chain_fb, "depth_fused_forward_backward": depth_fused_fb,
                                         "image_terms_operators_forward_backward": terms_chain_fb, "image_terms_fused_forward_backward": terms_fused_fb},
                                        reps, repeats)
            depth_stages = {name: t[len(t) // 2] for name, t in windows.items()}
            rec["depth_stage_windows_ms"] = {"calls_per_window": reps, "windows": windows}
            del rast_g
        normal_stages = {}
        if fit_normal != "off":
            # the normal term on its own, forward + backward, given the rasterisation each path starts from (as for the depth term),
            # and all image terms of this run with their rasterisation
            with_depth = fit_depth != "off"
            attr_g = (data._compute_vertex_normal() * torch.tensor([1, 1, -1], dtype=torch.float32, device=pos.device)[None, :]).detach().contiguous().requires_grad_(True)
            world_g = data.v_pos.detach().clone().requires_grad_(True)
            a_ref, a_ref3, n_ref = target[..., -1].contiguous(), target.contiguous(), target_normal.contiguous()
            rast_g, _ = dr.rasterize(ren.glctx, pos_g, tri, resolution=[res, res], grad_db=False)
            topo = dr.antialias_construct_topology_hash(tri)
            _, ids, _ = dr._silhouette_forward(pos, tri, topo.opp, ren.glctx, res, res)
            lib, check, stream = dr._lib, dr._capi.check, dr._stream_ptr(pos.device)
            B, V, T = int(pos.shape[0]), int(pos.shape[1]), int(tri.shape[0])
            ws = torch.empty(int(lib.tsamd_normal_mse_workspace_bytes(B * res * res)), dtype=torch.uint8, device=pos.device)
            loss_f, one = torch.empty((), device=pos.device), torch.ones((), device=pos.device)
            gn, gp = torch.empty_like(attr_g), torch.empty_like(pos)

            def normal_chain_fb(j):
                pos_g.grad = attr_g.grad = None
                n, _ = dr.interpolate(attr_g[None, ...], rast_g, tri)
                shade_loss(n * a_ref3, n_ref * a_ref3).backward(retain_graph=True)

            def normal_fused_fb(j):
                args = (pos.data_ptr(), B, V, tri.data_ptr(), T, res, res, ids.data_ptr(), attr_g.data_ptr(), n_ref.data_ptr(), a_ref.data_ptr())
                check(lib.tsamd_normal_mse(*args, ws.data_ptr(), loss_f.data_ptr(), None, stream))
                check(lib.tsamd_normal_mse_backward(*args, one.data_ptr(), 0, gn.data_ptr(), gp.data_ptr(), stream))

            def all_terms_chain_fb(j):
                pos_g.grad = attr_g.grad = world_g.grad = None
                r, _ = dr.rasterize(ren.glctx, pos_g, tri, resolution=[res, res], grad_db=False)
                a = dr.antialias(torch.clamp(r[..., -1:].detach(), 0, 1).contiguous(), r, pos_g, tri)
                n, _ = dr.interpolate(attr_g[None, ...], r, tri)
                total = shade_loss(a[..., -1], a_ref) * 20 + shade_loss(n * a_ref3, n_ref * a_ref3) * normal_weight
                if with_depth:
                    x, _ = dr.interpolate(world_g[None, ...], r, tri)
                    d = torch.norm(x - campos[:, None, None, :], dim=-1, keepdim=True)
                    total = total + shade_loss(d[..., -1] * a_ref, target_depth[..., -1] * a_ref) * 100
                total.backward()

            def all_terms_fused_fb(j):
                pos_g.grad = attr_g.grad = world_g.grad = None
                got = dr.silhouette_normal_mse(ren.glctx, pos_g, tri, [res, res], target, attr_g, target_normal, target,
                                               depth=(world_g, campos, target_depth, target) if with_depth else None)
                (got[0] * 20 + got[-1] * normal_weight + (got[1] * 100 if with_depth else 0)).backward()
            reps, repeats = normal_stage_reps
            windows = timed_alternating({"normal_operators_forward_backward": normal_chain_fb, "normal_fused_forward_backward": normal_fused_fb,
                                         "image_terms_operators_forward_backward": all_terms_chain_fb, "image_terms_fused_forward_backward": all_terms_fused_fb},
                                        reps, repeats)
            normal_stages = {name: t[len(t) // 2] for name, t in windows.items()}
            rec["normal_stage_windows_ms"] = {"calls_per_window": reps, "image_terms": "alpha, depth, normal" if with_depth else "alpha, normal", "windows": windows}
            del rast_g
        rec["stages_ms"] = {
            "energy_and_surface_forward_backward": timed(geo_fb),
            "rasterize": timed(lambda j: dr.rasterize(ren.glctx, pos, tri, resolution=[res, res], grad_db=False)),
            "antialias_forward_backward": timed(aa_fb),
            "silhouette_forward_backward": timed(sil_fb),
            "silhouette_mse_forward_backward": timed(sil_mse_fb),
            "optimizer_step": timed(lambda j: opt.step()),
            **depth_stages,
            **normal_stages,
        }
    return rec


def depth_bench(path, **kw):
    """Both --fit-depth modes on the same seed and the depth stage timings, as one record written to `path`."""
    kw = dict(kw, silhouette="fused-loss")
    ops = run(fit_depth="operators", stages=False, **kw)
    fused = run(fit_depth="fused-loss", stages=True, depth_stage_reps=(200, 5), **kw)
    w = fused["depth_stage_windows_ms"]["windows"]

    def pair(chain, own):
        return {"operators_ms": fused["stages_ms"][chain], "fused_ms": fused["stages_ms"][own], "operators_ms_min_max": [w[chain][0], w[chain][-1]],
                "fused_ms_min_max": [w[own][0], w[own][-1]], "ratio_operators_over_fused": fused["stages_ms"][chain] / fused["stages_ms"][own],
                "ranges_overlap": not (w[own][-1] < w[chain][0] or w[chain][-1] < w[own][0])}
    keep = ("ms_per_iteration", "silhouette_iou", "silhouette_iou_at_start", "inverted_tets", "img_loss_first_last", "fit_depth", "fit_depth_start", "iterations")
    rec = {"metric": "depth term forward + backward, operator chain over fused pair (medians of five windows of 200 calls, HIP events)",
           "value": fused["stages_ms"]["depth_operators_forward_backward"] / fused["stages_ms"]["depth_fused_forward_backward"], "unit": "x",
           "higher_is_better": True, "config": fused["config"],
           "depth_term": pair("depth_operators_forward_backward", "depth_fused_forward_backward"),
           "both_image_terms_with_their_rasterisation": pair("image_terms_operators_forward_backward", "image_terms_fused_forward_backward"),
           "windows_ms": fused["depth_stage_windows_ms"],
           "training": {"operators": {k: ops[k] for k in keep}, "fused-loss": {k: fused[k] for k in keep},
                        "ms_per_iteration_operators_over_fused": ops["ms_per_iteration"] / fused["ms_per_iteration"]},
           "stages_ms": fused["stages_ms"]}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    return rec


def normal_bench(path, **kw):
    """--fit-normal alone and together with --fit-depth, each in both modes on the same seed, and the normal stage timings, as one
    record written to `path`."""
    kw = dict(kw, silhouette="fused-loss")
    runs = {"normal": {"operators": run(fit_normal="operators", stages=False, **kw),
                       "fused-loss": run(fit_normal="fused-loss", stages=True, normal_stage_reps=(200, 5), **kw)},
            "depth_and_normal": {"operators": run(fit_normal="operators", fit_depth="operators", stages=False, **kw),
                                 "fused-loss": run(fit_normal="fused-loss", fit_depth="fused-loss", stages=True, normal_stage_reps=(200, 5), **kw)}}

    def pair(fused, chain, own):
        w = fused["normal_stage_windows_ms"]["windows"]
        return {"operators_ms": fused["stages_ms"][chain], "fused_ms": fused["stages_ms"][own], "operators_ms_min_max": [w[chain][0], w[chain][-1]],
                "fused_ms_min_max": [w[own][0], w[own][-1]], "ratio_operators_over_fused": fused["stages_ms"][chain] / fused["stages_ms"][own],
                "ranges_overlap": not (w[own][-1] < w[chain][0] or w[chain][-1] < w[own][0])}
    keep = ("ms_per_iteration", "silhouette_iou", "silhouette_iou_at_start", "inverted_tets", "img_loss_first_last", "fit_depth", "fit_depth_start", "fit_normal",
            "fit_normal_start", "normal_weight", "iterations")

    def training(modes):
        return {**{mode: {k: r[k] for k in keep} for mode, r in modes.items()},
                "ms_per_iteration_operators_over_fused": modes["operators"]["ms_per_iteration"] / modes["fused-loss"]["ms_per_iteration"]}
    alone, both = runs["normal"]["fused-loss"], runs["depth_and_normal"]["fused-loss"]
    term = pair(alone, "normal_operators_forward_backward", "normal_fused_forward_backward")
    rec = {"metric": "normal term forward + backward, operator chain over fused pair (medians of five windows of 200 calls, HIP events)",
           "value": term["ratio_operators_over_fused"], "unit": "x", "higher_is_better": True, "config": alone["config"],
           "normal_term": term,
           "alpha_and_normal_with_their_rasterisation": pair(alone, "image_terms_operators_forward_backward", "image_terms_fused_forward_backward"),
           "alpha_depth_and_normal_with_their_rasterisation": pair(both, "image_terms_operators_forward_backward", "image_terms_fused_forward_backward"),
           "windows_ms": {"normal": alone["normal_stage_windows_ms"], "depth_and_normal": both["normal_stage_windows_ms"]},
           "training": {"normal": training(runs["normal"]), "depth_and_normal": training(runs["depth_and_normal"])},
           "stages_ms": {"normal": alone["stages_ms"], "depth_and_normal": both["stages_ms"]}}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--target", default=None)
    ap.add_argument("--spheres", type=int, default=20)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--views", type=int, default=120)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--iters", type=int, default=1500)
    ap.add_argument("--verbose", action="store_true")
    ap.add_argument("--silhouette", choices=["operators", "fused", "fused-loss"], default="operators")
    ap.add_argument("--no-stages", action="store_true", help="skip the stand-alone stage timings")
    ap.add_argument("--fit-depth", choices=["off", "operators", "fused-loss"], default="off")
    ap.add_argument("--fit-depth-start", type=int, default=0, help="the depth term enters once the iteration has passed this one")
    ap.add_argument("--placement", choices=["host", "device", "mesh"], default="host",
                    help="place the tet-spheres with the host helper (default), with tssplat_amd.spheres_init from the silhouettes, or from the voxelised target mesh")
    ap.add_argument("--grid", type=int, default=72, help="voxels per axis of the placement grid")
    ap.add_argument("--merge-grid", type=int, default=0, metavar="N", help="merge the fitted spheres into one closed surface at N nodes per axis (0: off)")
    ap.add_argument("--merge-out", default=None, metavar="DIR", help="where merged_surface.obj goes (bench_outputs/train_object)")
    ap.add_argument("--merge-fill", choices=["none", "cavities", "outer"], default="none",
                    help="flood fill before the extraction: fill enclosed cavities, or also keep only the largest solid component")
    ap.add_argument("--merge-simplify", type=int, default=0, metavar="K",
                    help="cluster the merged surface on N // K cells per axis (tssplat_amd.simplify; 0: off, else an integer >= 2)")
    ap.add_argument("--merge-smooth", type=int, default=0, metavar="N",
                    help="smooth the merged surface by N iterations (tssplat_amd.smooth, both modes recorded, the default mode written; 0: off)")
    ap.add_argument("--eval-samples", type=int, default=0, metavar="N",
                    help="surface metrics (tssplat_amd.metrics.compare_meshes) of the raw, merged and filled surfaces against the target mesh on N samples each (0: off)")
    ap.add_argument("--eval-exact", action="store_true",
                    help="with --eval-samples: also `eval_exact`, the same surfaces with exact sample-to-triangle distances (tssplat_amd.metrics.compare_meshes_exact)")
    ap.add_argument("--eval-quality", action="store_true",
                    help="`eval_quality`: crossing pairs, topology and triangle shape (tssplat_amd.quality.mesh_quality) of the raw, merged, filled and simplified surfaces and the target")
    ap.add_argument("--eval-grid", type=int, default=0, metavar="N",
                    help="volume IoU (tssplat_amd.voxelize.mesh_volume_iou) of the raw, merged, filled and simplified surfaces against the target mesh at N nodes per axis (0: off)")
    ap.add_argument("--depth-bench", default=None, metavar="PATH", help="run both --fit-depth modes and the depth stage timings; write the record to PATH")
    ap.add_argument("--fit-normal", choices=["off", "operators", "fused-loss"], default="off")
    ap.add_argument("--fit-normal-start", type=int, default=0, help="the normal term enters once the iteration has passed this one")
    ap.add_argument("--normal-weight", type=float, default=100.0,
                    help="weight of the normal term (the reference's trainer has no normal line: the default mirrors its depth term's * 100)")
    ap.add_argument("--normal-bench", default=None, metavar="PATH",
                    help="run --fit-normal alone and with --fit-depth, each in both modes, and the normal stage timings; write the record to PATH")
    args = ap.parse_args()
    if args.normal_bench:
        rec = normal_bench(args.normal_bench, target_npz=args.target, n_spheres=args.spheres, k=args.k, views=args.views, res=args.res, iters=args.iters,
                           verbose=args.verbose, fit_depth_start=args.fit_depth_start, fit_normal_start=args.fit_normal_start, normal_weight=args.normal_weight,
                           placement=args.placement, grid=args.grid)
        print(json.dumps({k: rec[k] for k in ("metric", "value", "unit", "normal_term", "alpha_and_normal_with_their_rasterisation",
                                              "alpha_depth_and_normal_with_their_rasterisation", "training")}))
        return
    if args.depth_bench:
        rec = depth_bench(args.depth_bench, target_npz=args.target, n_spheres=args.spheres, k=args.k, views=args.views, res=args.res, iters=args.iters,
                          verbose=args.verbose, fit_depth_start=args.fit_depth_start, placement=args.placement, grid=args.grid)
        print(json.dumps({k: rec[k] for k in ("metric", "value", "unit", "depth_term", "both_image_terms_with_their_rasterisation", "training")}))
        return
    print(json.dumps(run(args.target, args.spheres, args.k, args.views, args.res, args.iters, verbose=args.verbose, silhouette=args.silhouette,
                         stages=not args.no_stages, fit_depth=args.fit_depth, fit_depth_start=args.fit_depth_start, fit_normal=args.fit_normal,
                         fit_normal_start=args.fit_normal_start, normal_weight=args.normal_weight, placement=args.placement, grid=args.grid,
                         merge_grid=args.merge_grid, merge_out=args.merge_out, merge_fill=args.merge_fill, eval_samples=args.eval_samples,
                         merge_simplify=args.merge_simplify, eval_grid=args.eval_grid, eval_exact=args.eval_exact, eval_quality=args.eval_quality,
                         merge_smooth=args.merge_smooth)))


if __name__ == "__main__":
    main()
