#!/usr/bin/env python3
"""The merge of the tet-spheres into one closed surface, stage by stage, on the mario fixture's 20 x kuhn8 scene.

The scene is what `tools/train_object.py --placement device` starts from: `spheres_init.init_spheres` on the 120 x 512^2 target
silhouettes of tests/golden/mario_mesh.npz, 20 spheres asked, `TetMeshMultiSphereGeometry(k=8)` -- the INITIAL spheres (the fitted ones come out of
`tools/train_object.py --merge-grid N`).  At every grid of `--grids` (128 and 256):

* `field`: `merge.union_field` (zero fill, the tet kernel, the decode pass);
* `count`: the count phase of the extraction, its two scans and the one readback of the totals;
* `emit`: the emit phase;
* `bake`: `atlas.bake_material` of an analytic colour field into the smallest power-of-two atlas >= 1024 that holds the triangles;
* `total`: `merge.merge_tets` end to end by the host clock, readbacks included.

Stage times are HIP events around the stage, the median of `--reps` runs after one warm-up.  Beside them: Nv, Nt, `closed`,
`inside_fraction`, and for the field stage the number of (tet, node) pairs it evaluates and the bytes it has to move at least
(one 4-byte read of the running maximum per pair, 12 bytes per node for the fill and the decode pass), so that its time can be
held against a bound.

The flood fill has a record of its own (--fill-out, profiles/merge_fill_bench.json), timed the same way at the same grids:
`labelling` (`merge.components`), `fill` (`merge.fill_field`, mode "cavities") and `fill_outer`, and next to them, for scale, the same
cavities fill by plain torch -- iterated masked neighbour-minimum sweeps until nothing changes, what a user would write without
the feature -- whose labels and field must equal the device's bit for bit.  Each row also holds the ratio to the sweeps, the ratio
to the same run's `count` stage (which reads the same field once), bytes per node, the four counts, and the components, surfaces,
Euler characteristic and handles of the extraction before and after.

    python tools/bench_merge.py [--grids 128 256 --reps 5 --out profiles/merge_bench.json --fill-out profiles/merge_fill_bench.json]

One JSON line on stdout; the whole records go to --out and --fill-out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def median_events(fn, reps):
    """(median milliseconds between two HIP events around `fn`, last result): `reps` calls after one warm-up."""
    import torch
    out = fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), out


def pair_count(tet_v, elem, grid, lo, hi):
    """(pairs, contributing tets): the box sizes of the contributing tets, as tests/union_oracle.py states them (numpy, float64)."""
    import numpy as np
    p = tet_v.astype(np.float64)[elem.astype(np.int64)]                      # [T, 4, 3]
    e1, e2, e3 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], p[:, 3] - p[:, 0]
    ok = np.isfinite(p).all(axis=(1, 2)) & (np.einsum("ij,ij->i", e1, np.cross(e2, e3)) > 0)
    h = (hi - lo) / grid
    first = np.maximum(np.ceil((p.min(1) - lo) / h - 0.5) - 1.0, 0.0)
    last = np.minimum(np.floor((p.max(1) - lo) / h - 0.5) + 1.0, grid - 1.0)
    size = np.clip(last - first + 1.0, 0.0, None).prod(1)
    return int(size[ok].sum()), int(ok.sum())


def torch_flood_labels(inside):
    """What a user would write without `merge.components`: the same labels by plain torch, iterated masked neighbour-minimum sweeps
    over the seven owned edges until nothing changes (one readback per sweep).  Each write takes the minimum with the CURRENT value:
    the two ends of an edge are overlapping views of one tensor.  Returns (labels int32 [G, G, G], sweeps)."""
    import torch
    G = inside.shape[0]
    lab = torch.arange(G ** 3, dtype=torch.int32, device=inside.device).reshape(G, G, G)
    big = torch.iinfo(torch.int32).max
    edges = []
    for m in range(1, 8):
        di, dj, dk = (m >> 2) & 1, (m >> 1) & 1, m & 1
        a, b = (slice(0, G - di), slice(0, G - dj), slice(0, G - dk)), (slice(di, G), slice(dj, G), slice(dk, G))
        edges.append((a, b, inside[a] == inside[b]))
    sweeps = 0
    while True:
        before = lab.clone()
        for a, b, same in edges:
            low = torch.where(same, torch.minimum(lab[a], lab[b]), big)
            lab[a] = torch.minimum(lab[a], low)
            lab[b] = torch.minimum(lab[b], low)
        sweeps += 1
        if bool((lab == before).all()):
            return lab, sweeps


def torch_fill_cavities(field, level):
    """`fill_field(field, level, "cavities").field` by plain torch, on the labels of the sweeps above."""
    import torch
    inside = field > level
    lab, sweeps = torch_flood_labels(inside)
    G = field.shape[0]
    border = torch.ones_like(inside)
    border[1:-1, 1:-1, 1:-1] = False
    exterior = torch.zeros(G ** 3, dtype=torch.bool, device=field.device)
    exterior[lab[border & ~inside].long()] = True
    cavity = ~inside & ~exterior[lab.reshape(-1).long()].reshape(G, G, G)
    return torch.where(cavity, torch.full_like(field, float("inf")), field), lab, sweeps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=120)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--spheres", type=int, default=20)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--grids", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_bench.json"))
    ap.add_argument("--fill-out", default=os.path.join(ROOT, "profiles", "merge_fill_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import train_object
    import tssplat_amd.dr as dr
    from tssplat_amd import atlas, geometry, merge, scenes, spheres_init

    assert torch.cuda.is_available(), "bench_merge.py needs a GPU"
    tgt = np.load(os.path.join(ROOT, "tests", "golden", "mario_mesh.npz"))
    tv = torch.from_numpy(tgt["vertices"].astype(np.float32)).cuda()
    tf = torch.from_numpy(tgt["faces"].astype(np.int32)).cuda()
    mvp = torch.from_numpy(scenes.dataset_mvps(args.views)).cuda()
    with torch.no_grad():
        target = train_object.render_alpha(dr.RasterizeCudaContext(), tv, tf, mvp, args.res).clone()
    kp = spheres_init.init_spheres(target, mvp, args.spheres, grid=72)
    geo = geometry.TetMeshMultiSphereGeometry(kp, k=args.k)
    tet_v, elem = geo.tet_v.detach().contiguous(), geo.tet_elem
    tet_v_h, elem_h = tet_v.cpu().numpy(), elem.cpu().numpy()

    class Field(torch.nn.Module):
        """The analytic colour field of tools/train_texture.py."""

        def forward(self, positions):
            return {"color": 0.5 + 0.5 * torch.sin(torch.stack([3.0 * positions[..., 0] + 1.0, 4.0 * positions[..., 1], 5.0 * positions[..., 2] - 0.5], -1))}
    material = Field()

    rec = {"metric": "merge of the tet-spheres into one closed surface, ms per stage", "unit": "ms", "higher_is_better": False,
           "config": {"workload": f"mario fixture, {len(kp)} tet-spheres x kuhn{args.k}: {int(elem.shape[0])} tets, {int(tet_v.shape[0])} vertices; "
                                  "initial spheres; bounds and level by default",
                      "timing": f"median of {args.reps} runs after one warm-up; HIP events around each stage, its readback included; total by the host clock"},
           "grids": {}}
    fill_rec = {"metric": "flood fill of the merged field: labelling and fill, ms", "unit": "ms", "higher_is_better": False,
                "config": {"workload": rec["config"]["workload"],
                           "timing": f"median of {args.reps} calls after one warm-up, HIP events around the call, its one readback included; "
                                     f"the torch sweeps: median of {min(args.reps, 3)}, one readback per sweep",
                           "stages": "labelling: merge.components; fill: merge.fill_field(mode='cavities') (labelling, marks, new field); fill_outer: mode='outer' "
                                     "(a second labelling, counts, the largest); count_stage: the extraction's count phase of the same run, which reads the same "
                                     "field once; torch_sweeps: the cavities fill by iterated masked neighbour-minimum sweeps in plain torch"},
                "grids": {}}
    for grid in args.grids:
        lo, hi = merge.default_bounds(tet_v, grid)
        level = merge.default_level(grid, (lo, hi))
        field_ms, field = median_events(lambda: merge.union_field(tet_v, elem, grid, (lo, hi)), args.reps)

        def count():
            vmask, vcount, tcount, flag = merge._count(field, level)
            vscan, tscan = torch.cumsum(vcount, 0, dtype=torch.int32), torch.cumsum(tcount, 0, dtype=torch.int32)
            nv, nt, is_open = (int(x) for x in torch.stack([vscan[-1], tscan[-1], flag[0]]).cpu().numpy())
            return vmask, vscan - vcount, tscan - tcount, nv, nt, is_open
        count_ms, (vmask, voffset, toffset, nv, nt, is_open) = median_events(count, args.reps)
        emit_ms, (v, faces) = median_events(lambda: merge._emit(field, lo, hi, level, vmask, voffset, toffset, nv, nt), args.reps)
        tex_res = 1024
        while True:
            try:
                atlas.atlas_layout(nt, tex_res)
                break
            except ValueError:
                tex_res *= 2
        bake_ms, _ = median_events(lambda: atlas.bake_material(material, v, faces, tex_res), args.reps)
        walls = []
        for _ in range(args.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            merged = merge.merge_tets(tet_v, elem, grid=grid)
            torch.cuda.synchronize()
            walls.append(1e3 * (time.perf_counter() - t0))
        pairs, contributing = pair_count(tet_v_h, elem_h, grid, lo, hi)
        nodes = grid ** 3
        bytes_min = 4 * pairs + 12 * nodes
        row = {"bounds": [lo, hi], "level": level, "stages_ms": {"field": field_ms, "count": count_ms, "emit": emit_ms, "bake": bake_ms},
               "merge_tets_wall_ms": statistics.median(walls[1:]), "vertices": nv, "triangles": nt, "closed": not is_open, "inside_fraction": merged.inside_fraction,
               "texture_res": tex_res,
               "field_stage": {"contributing_tets": contributing, "tet_node_pairs": pairs, "pairs_per_tet": pairs / max(1, contributing), "nodes": nodes,
                               "bytes_at_least": bytes_min, "note": "4 bytes read per pair (the running maximum) + 12 bytes per node (fill, decode read and write)",
                               "pairs_per_us": pairs / (1e3 * field_ms), "GB_per_s_at_least": bytes_min / (1e6 * field_ms),
                               "float64_adds_and_multiplies_per_pair": 35, "GFLOP64_per_s": 35 * pairs / (1e6 * field_ms)}}
        assert merged.closed == (not is_open) and int(merged.v.shape[0]) == nv and int(merged.faces.shape[0]) == nt
        rec["grids"][str(grid)] = row

        # ---- the flood fill: the labelling alone, the fill in both modes, and the same by plain torch for scale ----
        label_ms, label = median_events(lambda: merge.components(field, level), args.reps)
        modes = {}
        for mode in ("cavities", "outer"):
            ms, filled = median_events(lambda: merge.fill_field(field, level, mode), args.reps)
            fv, ff, fclosed = merge.extract_surface(filled.field, (lo, hi), level)
            modes[mode] = {"ms": ms, "cavities": filled.cavities, "cavity_nodes": filled.cavity_nodes, "islands": filled.islands,
                           "island_nodes": filled.island_nodes, "vertices": int(fv.shape[0]), "triangles": int(ff.shape[0]), "closed": fclosed,
                           **train_object.surface_topology(filled.field, level, fv.shape[0], ff.shape[0])}
            if mode == "cavities":
                cavities_field = filled.field
        torch_ms, (torch_field, torch_label, sweeps) = median_events(lambda: torch_fill_cavities(field, level), min(args.reps, 3))
        assert torch.equal(torch_label, label), "the torch sweeps and merge.components disagree"
        assert torch_field.cpu().numpy().tobytes() == cavities_field.cpu().numpy().tobytes(), "the torch fill and merge.fill_field disagree"
        fill_ms = modes["cavities"]["ms"]
        fill_row = {"labelling_ms": label_ms, "fill_ms": fill_ms, "fill_outer_ms": modes["outer"]["ms"], "count_stage_ms": count_ms,
                    "torch_sweeps_ms": torch_ms, "torch_sweeps": sweeps, "torch_sweeps_over_fill": torch_ms / fill_ms, "fill_over_count_stage": fill_ms / count_ms,
                    "labelling_over_count_stage": label_ms / count_ms, "nodes": nodes,
                    "bytes_per_node": {"held": 16, "held_note": "field 4 + new field 4 + workspace 8 (labels, marks / counts)",
                                       "moved_at_least_labelling": 16, "moved_at_least_fill": 32,
                                       "moved_note": "labelling: field read 4, label written 4, flatten read and write 8; the cavities fill adds field 4, label 4, "
                                                     "mark 4 and the new field 4 (the merge pass over tile faces and every retry come on top)",
                                       "GB_per_s_at_least_labelling": 16 * nodes / (1e6 * label_ms), "GB_per_s_at_least_fill": 32 * nodes / (1e6 * fill_ms)},
                    "unfilled": {"vertices": nv, "triangles": nt, **train_object.surface_topology(field, level, nv, nt)},
                    "cavities": modes["cavities"], "outer": modes["outer"]}
        fill_rec["grids"][str(grid)] = fill_row
        print(f"grid {grid} fill: {json.dumps(fill_row)}", file=sys.stderr, flush=True)
        print(f"grid {grid}: {json.dumps(row)}", file=sys.stderr, flush=True)
    first = rec["grids"][str(args.grids[0])]
    rec["value"] = first["merge_tets_wall_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    fill_rec["value"] = fill_rec["grids"][str(args.grids[0])]["fill_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(args.fill_out)), exist_ok=True)
    with open(args.fill_out, "w") as fh:
        json.dump(fill_rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: rec[k] for k in ("metric", "value", "unit")} | {"grids": {g: r["stages_ms"] | {"vertices": r["vertices"], "triangles": r["triangles"],
                                                                                                            "closed": r["closed"]} for g, r in rec["grids"].items()}}))


if __name__ == "__main__":
    main()
