#!/usr/bin/env python3
"""The mesh-quality stage, timed: `quality`'s prepare pass, the crossing-pair search in both orders and the topology, on the mario
target mesh, the mario scene merged at grid 128 and 256 and the raw union of its 20 kuhn8 sphere boundaries.

    python tools/bench_quality.py [--reps 7 --baseline-reps 3 --grids 128 256 --out profiles/quality_bench.json]

Timing: HIP events around each call after one warm-up, medians of --reps with their minimum and maximum; run it in a fresh process.
`search_flat` is `tsamd_quality_pairs` without tile boxes; `search_morton` is everything `order="morton"` adds to it: the sort of the
Morton keys, the three gathers and `tsamd_quality_pairs` with tile boxes.  Both write `crossings`, whose SHA-256 (mapped back to the
caller's order) the record holds, and the bench asserts that the two and the sorted pair lists are equal.

The baseline is the same integers in plain torch on the same GPU: a block of rows i against all j at a time, the box test on the
unpacked int32 lattice boxes, `nonzero`, and the six segment / triangle tests in int64 on the survivors.  It runs on the first rows
only where all of them would take too long (--baseline-pairs box tests at most), its time scaled by the share of the pairs i < j
those rows hold, and must list exactly the device's crossing pairs with i in those rows.

One JSON line on stdout; the whole record goes to --out."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_metrics import median_events  # noqa: E402


def torch_crossing_pairs(corners, state, rows_total, budget=1 << 27):
    """The baseline: (sorted keys i << 32 | j of the crossing pairs with i < rows_total, box pairs among them)."""
    import torch
    T = int(corners.shape[0])
    good = state == 0
    X = torch.stack([corners & 0xFFFFF, (corners >> 21) & 0xFFFFF, (corners >> 42) & 0xFFFFF], dim=2)      # [T, 3 corners, 3 axes]
    X = torch.where(good[:, None, None], X, torch.zeros_like(X))
    bmin, bmax = X.min(dim=1).values.int(), X.max(dim=1).values.int()
    ids = torch.arange(T, device=corners.device)

    def cross(u, v):
        return torch.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], dim=1)

    def orient(a, b, c, d):
        return ((b - a) * cross(c - a, d - a)).sum(dim=1)

    def pierces(p, q, a, b, c):
        sp, sq = orient(a, b, c, p), orient(a, b, c, q)
        o1, o2, o3 = orient(p, q, a, b), orient(p, q, b, c), orient(p, q, c, a)
        return (((sp > 0) & (sq < 0)) | ((sp < 0) & (sq > 0))) & (((o1 > 0) & (o2 > 0) & (o3 > 0)) | ((o1 < 0) & (o2 < 0) & (o3 < 0)))

    rows = max(1, budget // T)
    keys, boxes = [], 0
    for r0 in range(0, rows_total, rows):
        r1 = min(rows_total, r0 + rows)
        ov = good[r0:r1, None] & good[None, :] & (ids[None, :] > ids[r0:r1, None])
        for k in range(3):
            ov &= (bmin[r0:r1, None, k] <= bmax[None, :, k]) & (bmin[None, :, k] <= bmax[r0:r1, None, k])
        i, j = torch.nonzero(ov, as_tuple=True)
        i = i + r0
        boxes += int(i.shape[0])
        A, B = X[i], X[j]
        hit = torch.zeros(i.shape[0], dtype=torch.bool, device=corners.device)
        for k in range(3):
            hit |= pierces(A[:, k], A[:, (k + 1) % 3], B[:, 0], B[:, 1], B[:, 2])
            hit |= pierces(B[:, k], B[:, (k + 1) % 3], A[:, 0], A[:, 1], A[:, 2])
        keys.append((i[hit] << 32) | j[hit])
    return torch.sort(torch.cat(keys))[0], boxes


def quality_kernels(lib):
    """kernel -> registers, scratch and LDS, from the code object's metadata."""
    import re
    import kernel_metadata
    out = {}
    for k, v in kernel_metadata.kernel_metadata(lib).items():
        m = re.search(r"\d(quality_[a-z_]+_kernel|union_(?:init|hook|compress)_kernel)", k)
        if m:
            out[m.group(1)] = {"vgpr_count": v["vgpr_count"], "sgpr_count": v["sgpr_count"], "scratch_bytes": v["private_segment_fixed_size"],
                               "lds_bytes": v["group_segment_fixed_size"]}
    return out


def sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def bench_mesh(name, v, f, args):
    import torch
    from tssplat_amd import quality
    T = int(f.shape[0])
    lo, hi = quality._bounds("bench", v, f, None)
    cap = args.max_pairs
    prep_ms, prep_span, prepared = median_events(lambda: quality._prepare(v, f, lo, hi), args.reps)
    corners, boxes, state, _, morton = prepared
    flat_ms, flat_span, (cr_flat, pairs_flat, stats_flat) = median_events(lambda: quality._pairs(corners, boxes, state, cap, False), args.reps)

    def morton_search():
        perm = torch.sort(morton)[1]
        out = quality._pairs(corners[perm].contiguous(), boxes[perm].contiguous(), state[perm].contiguous(), cap, True)
        return perm, out
    mort_ms, mort_span, (perm, (cr_m, pairs_m, stats_m)) = median_events(morton_search, args.reps)
    sort_ms, _, _ = median_events(lambda: torch.sort(morton)[1], args.reps)
    topo_ms, topo_span, topo = median_events(lambda: quality._topology(f, state, int(v.shape[0])), args.reps)
    sf, sm = (dict(zip(quality._STATS, (int(x) for x in s.cpu().numpy()))) for s in (stats_flat, stats_m))
    n = sf["crossing_pairs"]
    assert n <= cap, f"{name}: {n} crossing pairs overflow --max-pairs {cap}"
    cr_back = torch.zeros_like(cr_m).scatter_(0, perm, cr_m)
    i, j = perm[pairs_m[:n] >> 32], perm[pairs_m[:n] & 0xFFFFFFFF]
    keys_m = torch.sort((torch.minimum(i, j) << 32) | torch.maximum(i, j))[0]
    keys_flat = torch.sort(pairs_flat[:n])[0]
    same = {k: sf[k] == sm[k] for k in ("crossing_pairs", "crossing_faces", "invalid_faces", "degenerate_faces", "box_pairs")}
    assert all(same.values()) and torch.equal(cr_flat, cr_back) and torch.equal(keys_flat, keys_m), f"{name}: the two orders disagree: {sf} {sm}"
    # the torch statement, on the first rows where all of them are too many
    rows = T if T * T <= args.baseline_pairs else max(1, min(T, args.baseline_pairs // T))
    base_ms, base_span, (base_keys, base_boxes) = median_events(lambda: torch_crossing_pairs(corners, state, rows), args.baseline_reps)
    assert torch.equal(base_keys, keys_flat[(keys_flat >> 32) < rows]), f"{name}: the kernel and the torch statement disagree"
    share = (rows * (2 * T - rows - 1) / 2) / (T * (T - 1) / 2) if T > 1 else 1.0
    base_all = base_ms / share
    pairs_all = T * (T - 1) / 2
    q = quality.mesh_quality(v, f).as_dict()
    return {"triangles": T, "vertices": int(v.shape[0]), "bounds": [lo, hi], "prepare_ms": prep_ms, "prepare_ms_min_max": prep_span,
            "search_flat_ms": flat_ms, "search_flat_ms_min_max": flat_span, "search_morton_ms": mort_ms, "search_morton_ms_min_max": mort_span,
            "of_which_sort_ms": sort_ms, "topology_ms": topo_ms, "topology_ms_min_max": topo_span, "union_rounds": list(topo.union_rounds),
            "box_pairs": sf["box_pairs"], "crossing_pairs": n, "crossing_faces": sf["crossing_faces"], "invalid_faces": sf["invalid_faces"],
            "degenerate_faces": sf["degenerate_faces"], "tile_visits_flat": sf["tile_visits"], "tile_visits_morton": sm["tile_visits"],
            "pairs_per_s_flat": pairs_all / (flat_ms * 1e-3), "pairs_per_s_morton": pairs_all / (mort_ms * 1e-3), "flat_over_morton": flat_ms / mort_ms,
            "morton_faster_beyond_spread": mort_span[1] < flat_span[0], "crossings_sha256_flat": sha(cr_flat), "crossings_sha256_morton": sha(cr_back),
            "pairs_sha256": sha(keys_flat), "torch_rows": rows, "torch_box_pairs_in_rows": base_boxes, "torch_ms": base_ms, "torch_ms_min_max": base_span,
            "torch_share_of_pairs": share, "torch_ms_scaled_to_all_rows": base_all, "torch_over_flat": base_all / flat_ms, "torch_over_morton": base_all / mort_ms,
            "device_faster_than_torch_beyond_spread": base_span[0] / share > max(flat_span[1], mort_span[1]), "pairs_identical_to_torch": True, "quality": q}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--baseline-reps", type=int, default=3)
    ap.add_argument("--grids", type=int, nargs="*", default=[128, 256])
    ap.add_argument("--max-pairs", type=int, default=1 << 23)
    ap.add_argument("--baseline-pairs", type=int, default=4 * 10 ** 9, help="box tests of the torch statement at most; fewer rows beyond")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quality_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import train_object
    import tssplat_amd.dr as dr
    from tssplat_amd import _capi, geometry, merge, quality, scenes, spheres_init

    assert torch.cuda.is_available(), "bench_quality.py needs a GPU"
    tgt = np.load(os.path.join(ROOT, "tests", "golden", "mario_mesh.npz"))
    tv = torch.from_numpy(tgt["vertices"].astype(np.float32)).cuda()
    tf = torch.from_numpy(tgt["faces"].astype(np.int32)).cuda()
    mvp = torch.from_numpy(scenes.dataset_mvps(120)).cuda()
    with torch.no_grad():
        target = train_object.render_alpha(dr.RasterizeCudaContext(), tv, tf, mvp, 512).clone()
    kp = spheres_init.init_spheres(target, mvp, 20, grid=72)
    geo = geometry.TetMeshMultiSphereGeometry(kp, k=8)
    info = quality.launch_info()
    try:
        kernels = quality_kernels(_capi.lib_path())
    except Exception as exc:                                              # the LLVM tools are not there
        kernels = {"unavailable": repr(exc)}
    rec = {"metric": "crossing-pair search of the largest mesh, plain torch over the default order", "unit": "x", "higher_is_better": True,
           "config": {"timing": f"HIP events around each call after one warm-up; medians of {args.reps} calls ({args.baseline_reps} for the torch statement), one process",
                      "block": info["block"], "tile": info["tile"], "queue": info["queue"], "default_order": quality.DEFAULT_ORDER, "kernels": kernels,
                      "workload": f"mario fixture: the target mesh; {len(kp)} initial tet-spheres x kuhn8, their raw union and their merge at grids {args.grids}"},
           "meshes": {}}
    meshes = [("mario_target", tv, tf), ("raw_union_20_kuhn8", geo.tet_v.detach()[geo.surface_vid.long()].contiguous(), geo.surface_fid.contiguous())]
    for g in args.grids:
        m = merge.merge_tets(geo.tet_v.detach().contiguous(), geo.tet_elem, grid=g)
        meshes.append((f"merged_grid_{g}", m.v, m.faces))
    for name, v, f in meshes:
        rec["meshes"][name] = bench_mesh(name, v, f, args)
        print(name, json.dumps({k: rec["meshes"][name][k] for k in ("triangles", "prepare_ms", "search_flat_ms", "search_morton_ms", "topology_ms", "box_pairs",
                                                                     "crossing_pairs", "torch_over_flat", "torch_over_morton")}), file=sys.stderr, flush=True)
    last = rec["meshes"][meshes[-1][0]]
    rec["value"] = last["torch_over_morton" if quality.DEFAULT_ORDER == "morton" else "torch_over_flat"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"metric": rec["metric"], "value": rec["value"], "unit": "x",
                      "meshes": {k: {x: m[x] for x in ("triangles", "search_flat_ms", "search_morton_ms", "flat_over_morton", "torch_over_flat")} for k, m in rec["meshes"].items()}}))


if __name__ == "__main__":
    main()
