#!/usr/bin/env python
"""Stage timings of the surface simplifier (tssplat_amd.simplify) on the merged mario fixture, on one GPU.

Workload and protocol are tools/bench_merge.py's: the mario fixture's 20 x kuhn8 tet-spheres as `spheres_init.init_spheres` places them,
merged at --grids nodes per axis; median of --reps runs after one warm-up, HIP events around each stage, readbacks included.  Per grid
and --factors k (cells = grid // k): the stages keys, sort, run walk, faces (triples, two stable sorts, duplicate flags) and compaction
(the one readback and the scans), the counts before and after, `edge_stats`, `clamped`, `duplicates`, the run lengths, and the
run walk's gathered bytes against its time.

Two comparisons go into the same record:
  torch      the same clustering in plain torch (`index_add_` on float64, `torch.linalg.solve`) on the same input: its time, whether two
             runs of it agree bit for bit, and how far its positions are from the kernels'
  coarser    `metrics.compare_meshes` against the unsimplified mesh of the finest grid, at --samples samples with `noise_floor`, of
             (a) that mesh simplified by the largest factor and (b) `merge_tets` at grid // factor nodes -- the lighter mesh a user could
             get before this module existed.  Whatever comes out is recorded, including (b) winning

    python tools/bench_simplify.py [--grids 128 256 --factors 2 4 --reps 5 --samples 100000 --out profiles/simplify_bench.json]

One JSON line on stdout; the whole record goes to --out."""
import argparse
import dataclasses
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

RECORD_BYTES = {"record": 8, "perm": 8, "face": 12, "vertex_keys": 12, "corners": 36, "run": 4}      # what the run walk gathers and writes per record


def torch_cluster(v, faces, cells, lo, hi, stabilise):
    """The clustering a user would write in plain torch: float64 `index_add_` sums per cell and a batched `torch.linalg.solve`.  Same
    formulas as tests/simplify_oracle.py, but the sums' order is whatever `index_add_` does (atomics).  Valid input only.
    -> (cell keys [K], positions float32 [K, 3], kept faces as cell-key triples)"""
    import torch
    C = cells
    h = (hi - lo) / C
    p = v.double()
    idx = torch.clamp(torch.floor((p - lo) / h), 0, C - 1).long()
    vkey = (idx[:, 0] * C + idx[:, 1]) * C + idx[:, 2]
    f = faces.long()
    fk = vkey[f]                                                             # [T, 3]
    ucell, inv = torch.unique(vkey[f.reshape(-1)], return_inverse=True)
    inv = inv.reshape(-1, 3)
    K = int(ucell.shape[0])
    g = lo + (torch.stack([ucell // (C * C), (ucell // C) % C, ucell % C], 1).double() + 0.5) * h
    a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    n = torch.cross(b - a, c - a, dim=1)
    A = torch.zeros((K, 3, 3), dtype=torch.float64, device=v.device)
    bb = torch.zeros((K, 3), dtype=torch.float64, device=v.device)
    P = torch.zeros((K, 3), dtype=torch.float64, device=v.device)
    cnt = torch.zeros(K, dtype=torch.float64, device=v.device)
    nnT = n[:, :, None] * n[:, None, :]
    for s in range(3):                                                       # one record per distinct cell of the face
        new = torch.ones_like(inv[:, 0], dtype=torch.bool)
        for e in range(s):
            new &= inv[:, e] != inv[:, s]
        cell = inv[new, s]
        d = -(n[new] * (a[new] - g[cell])).sum(1)
        A.index_add_(0, cell, nnT[new])
        bb.index_add_(0, cell, d[:, None] * n[new])
        corner = (a, b, c)[s]
        P.index_add_(0, inv[:, s], corner - g[inv[:, s]])
        cnt.index_add_(0, inv[:, s], torch.ones_like(cnt[inv[:, s]]))
    m = P / cnt[:, None]
    tr = A.diagonal(dim1=1, dim2=2).sum(1)
    lam = stabilise * tr
    M = A + lam[:, None, None] * torch.eye(3, dtype=torch.float64, device=v.device)
    good = tr > 0
    M = torch.where(good[:, None, None], M, torch.eye(3, dtype=torch.float64, device=v.device).expand_as(M))
    x = torch.linalg.solve(M, (lam[:, None] * m - bb)[:, :, None])[:, :, 0]
    x = torch.where((good & torch.isfinite(x).all(1))[:, None], x, m).clamp(-0.5 * h, 0.5 * h)
    keep = (fk[:, 0] != fk[:, 1]) & (fk[:, 0] != fk[:, 2]) & (fk[:, 1] != fk[:, 2])
    return ucell, (g + x).float(), fk[keep]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=120)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--spheres", type=int, default=20)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--grids", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--factors", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--samples", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplify_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import train_object
    import tssplat_amd.dr as dr
    from bench_merge import median_events
    from tssplat_amd import geometry, merge, metrics, scenes, simplify, spheres_init

    assert torch.cuda.is_available(), "bench_simplify.py needs a GPU"
    tgt = np.load(os.path.join(ROOT, "tests", "golden", "mario_mesh.npz"))
    tv = torch.from_numpy(tgt["vertices"].astype(np.float32)).cuda()
    tf = torch.from_numpy(tgt["faces"].astype(np.int32)).cuda()
    mvp = torch.from_numpy(scenes.dataset_mvps(args.views)).cuda()
    with torch.no_grad():
        target = train_object.render_alpha(dr.RasterizeCudaContext(), tv, tf, mvp, args.res).clone()
    kp = spheres_init.init_spheres(target, mvp, args.spheres, grid=72)
    geo = geometry.TetMeshMultiSphereGeometry(kp, k=args.k)
    tet_v, elem = geo.tet_v.detach().contiguous(), geo.tet_elem
    stab = simplify.DEFAULT_STABILISE

    rec = {"metric": "surface simplification (vertex clustering, quadric placement) of the merged surface, ms per stage", "unit": "ms", "higher_is_better": False,
           "config": {"workload": f"mario fixture, {len(kp)} tet-spheres x kuhn{args.k}: {int(elem.shape[0])} tets; initial spheres; merge bounds and level by default",
                      "timing": f"median of {args.reps} runs after one warm-up; HIP events around each stage, its readback included",
                      "stages": "keys: cell keys and record slots; sort: torch.sort of the 64-bit records; run_walk: the per-cell sums and solve; faces: triples, two "
                                "stable sorts, duplicate flags and used marks; compaction: the one readback, the scan, the gathers",
                      "bytes_per_record": RECORD_BYTES},
           "grids": {}}
    meshes = {}
    for grid in args.grids:
        merged = merge.merge_tets(tet_v, elem, grid=grid)
        v, faces, (lo, hi) = merged.v, merged.faces, merged.bounds
        meshes[grid] = merged
        rows = {}
        for k in args.factors:
            cells = grid // k
            status = torch.zeros(2, dtype=torch.int32, device=v.device)
            keys_ms, (vkey, records, state) = median_events(lambda: simplify._keys(v, faces, cells, lo, hi), args.reps)
            sort_ms, (records, perm) = median_events(lambda: tuple(torch.sort(records)), args.reps)
            walk_ms, (pos, head, run) = median_events(lambda: simplify._cells(v, faces, cells, lo, hi, "quadric", stab, vkey, records, perm, status[0:1]), args.reps)
            faces_ms, (tri, keep, used) = median_events(lambda: simplify._faces(run, state, status[1:2]), args.reps)
            compact_ms, (out_v, out_f, counts) = median_events(lambda: simplify._compact("simplify", pos, head, state, tri, keep, used, status), args.reps)
            total_ms, simp = median_events(lambda: simplify.simplify(v, faces, cells, (lo, hi)), args.reps)
            assert torch.equal(simp.v.view(torch.int32), out_v.view(torch.int32)) and torch.equal(simp.faces, out_f)
            lengths = simplify.run_lengths(v, faces, cells, (lo, hi)).cpu().numpy()
            n_records = int(lengths.sum())
            walk_bytes = n_records * sum(RECORD_BYTES.values())
            hist = np.bincount(np.minimum(np.ceil(np.log2(np.maximum(lengths, 1))).astype(np.int64), 16))
            # the same in plain torch
            torch_ms, (tcell, tpos, tfaces) = median_events(lambda: torch_cluster(v, faces, cells, lo, hi, stab), args.reps)
            again = torch_cluster(v, faces, cells, lo, hi, stab)[1]
            ours = pos[head != 0]
            row = {"cells": cells, "stages_ms": {"keys": keys_ms, "sort": sort_ms, "run_walk": walk_ms, "faces": faces_ms, "compaction": compact_ms},
                   "stages_sum_ms": keys_ms + sort_ms + walk_ms + faces_ms + compact_ms, "simplify_ms": total_ms,
                   "vertices_before": int(v.shape[0]), "triangles_before": int(faces.shape[0]), "vertices_after": int(simp.v.shape[0]),
                   "triangles_after": int(simp.faces.shape[0]), "cells_occupied": simp.cells_occupied, "clamped": simp.clamped, "duplicates": simp.duplicates,
                   "degenerate_faces": simp.degenerate_faces, "invalid_faces": simp.invalid_faces, "edge_stats": dataclasses.asdict(simplify.edge_stats(simp.faces)),
                   "run_lengths": {"records": n_records, "mean": float(lengths.mean()), "median": float(np.median(lengths)), "p99": float(np.percentile(lengths, 99)),
                                   "max": int(lengths.max()), "runs_by_ceil_log2_length": hist.tolist()},
                   "run_walk": {"bytes_gathered": walk_bytes, "GB_per_s": walk_bytes / (1e6 * walk_ms), "records_per_us": n_records / (1e3 * walk_ms)},
                   "torch": {"ms": torch_ms, "over_simplify": torch_ms / total_ms, "repeats_bitwise": bool(torch.equal(again.view(torch.int32), tpos.view(torch.int32))),
                             "cells_agree": bool(tcell.shape[0] == ours.shape[0]), "surviving_faces_agree": bool(tfaces.shape[0] == simp.faces.shape[0] + simp.duplicates),
                             "max_abs_position_difference": float((tpos - ours).abs().max()) if tcell.shape[0] == ours.shape[0] else None,
                             "positions_equal_bitwise": bool(tcell.shape[0] == ours.shape[0] and torch.equal(tpos.view(torch.int32), ours.view(torch.int32)))}}
            rows[str(k)] = row
            print(f"grid {grid} simplify {k}: {json.dumps(row)}", file=sys.stderr, flush=True)
        rec["grids"][str(grid)] = rows

    # ---- against a coarser merge grid: which lighter mesh is closer to the fine one? ----
    fine, k = max(args.grids), max(args.factors)
    ref = meshes[fine]
    a = simplify.simplify(ref.v, ref.faces, fine // k, ref.bounds)
    b = merge.merge_tets(tet_v, elem, grid=fine // k)
    cmp_a = metrics.compare_meshes(a.v, a.faces, ref.v, ref.faces, n=args.samples, seed=0).as_dict()
    cmp_b = metrics.compare_meshes(b.v, b.faces, ref.v, ref.faces, n=args.samples, seed=0).as_dict()
    rec["against_coarser_grid"] = {"reference": f"merge_tets at grid {fine}, unsimplified: {int(ref.faces.shape[0])} triangles", "samples": args.samples,
                                   "simplified": {"what": f"grid {fine}, simplify={k}", "triangles": int(a.faces.shape[0]), "vertices": int(a.v.shape[0]), **cmp_a},
                                   "coarser_grid": {"what": f"merge_tets at grid {fine // k}", "triangles": int(b.faces.shape[0]), "vertices": int(b.v.shape[0]), **cmp_b},
                                   "simplified_wins_chamfer_l1": bool(cmp_a["chamfer_l1"] < cmp_b["chamfer_l1"])}
    head_row = rec["grids"][str(fine)][str(k)]
    rec["value"] = head_row["simplify_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"metric": rec["metric"], "value": rec["value"], "unit": "ms", "grid": fine, "simplify": k, "triangles_before": head_row["triangles_before"],
                      "triangles_after": head_row["triangles_after"], "torch_over_simplify": head_row["torch"]["over_simplify"],
                      "simplified_chamfer_l1": cmp_a["chamfer_l1"], "coarser_grid_chamfer_l1": cmp_b["chamfer_l1"], "noise_floor": cmp_a["noise_floor"]}))


if __name__ == "__main__":
    main()
