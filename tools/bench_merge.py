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

    python tools/bench_merge.py [--grids 128 256 --reps 5 --out profiles/merge_bench.json]

One JSON line on stdout; the whole record goes to --out."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=120)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--spheres", type=int, default=20)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--grids", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_bench.json"))
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
        print(f"grid {grid}: {json.dumps(row)}", file=sys.stderr, flush=True)
    first = rec["grids"][str(args.grids[0])]
    rec["value"] = first["merge_tets_wall_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: rec[k] for k in ("metric", "value", "unit")} | {"grids": {g: r["stages_ms"] | {"vertices": r["vertices"], "triangles": r["triangles"],
                                                                                                            "closed": r["closed"]} for g, r in rec["grids"].items()}}))


if __name__ == "__main__":
    main()
