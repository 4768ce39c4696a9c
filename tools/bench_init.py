#!/usr/bin/env python3
"""Sphere placement on the device against the host helper, on the silhouettes of the mario fixture.

`tssplat_amd.spheres_init.init_spheres` (HIP: bit-packed occupancy, hull carve, separable squared distance transform, greedy cover)
against `tools/train_object.py::place_spheres` (a torch loop over the views, scipy's distance transform, a numpy loop) on the
same 120 x 512^2 target alpha images, 20 spheres asked.  Every time is end to end, the final readback included: the median of
`--reps` runs after one warm-up, a host clock around work that ends in a device synchronise.  The device path is timed at
`--grids` (72 and 192); the host path at 72 and, where it fits, at the larger grids too.  The device stages (pack, carve, EDT,
cover) are timed on their own with HIP events -- pack as a hull call on one voxel that the first view rejects, carve as the hull
call minus that.

Then the fit itself: `tools/train_object.py` with `--placement host` and `--placement device` in this session (spheres placed,
final silhouette IoU; the recorded 0.971 of profiles/r06_train_mario.json beside them).

    python tools/bench_init.py [--views 120 --res 512 --spheres 20 --grids 72 192 --reps 5 --iters 1500 --no-train --out profiles/init_bench.json]

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


def median_wall(fn, reps):
    """(median seconds, all seconds, last result) of `reps` calls after one warm-up; every call ends synchronised."""
    import torch
    fn()
    torch.cuda.synchronize()
    times, out = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), times, out


def median_events(fn, reps):
    """Median milliseconds between two HIP events around `fn`, `reps` calls after one warm-up."""
    import torch
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=120)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--spheres", type=int, default=20)
    ap.add_argument("--grids", type=int, nargs="+", default=[72, 192])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=1500)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--no-train", action="store_true", help="skip the two fits")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "init_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import train_object
    import tssplat_amd.dr as dr
    from tssplat_amd import scenes, spheres_init

    assert torch.cuda.is_available(), "bench_init.py needs a GPU"
    tgt = np.load(os.path.join(ROOT, "tests", "golden", "mario_mesh.npz"))
    tv = torch.from_numpy(tgt["vertices"].astype(np.float32)).cuda()
    tf = torch.from_numpy(tgt["faces"].astype(np.int32)).cuda()
    mvp = torch.from_numpy(scenes.dataset_mvps(args.views)).cuda()
    with torch.no_grad():
        target = train_object.render_alpha(dr.RasterizeCudaContext(), tv, tf, mvp, args.res).clone()

    rec = {"metric": "sphere placement end to end (readback included), host helper over device path at grid 72", "unit": "x", "higher_is_better": True,
           "config": {"workload": f"mario fixture, {args.views} views x {args.res}^2 target alpha, {args.spheres} spheres asked, min_radius 0.05, shrink 0.92",
                      "timing": f"median of {args.reps} runs after one warm-up; wall clock around synchronised work; stages by HIP events"},
           "grids": {}}
    for grid in args.grids:
        row = {}
        t, all_t, kp = median_wall(lambda: spheres_init.init_spheres(target, mvp, args.spheres, grid=grid), args.reps)
        row["device"] = {"ms": 1e3 * t, "ms_all": [1e3 * x for x in all_t], "spheres": len(kp), "hull_fraction": kp.hull_fraction,
                         "uncovered_fraction": kp.uncovered_fraction, "radii_min_max": [float(kp.r.min()), float(kp.r.max())] if len(kp) else None}
        # the stages on their own
        pack = median_events(lambda: spheres_init.visual_hull(target, mvp, grid=1, bounds=(50.0, 51.0)), args.reps)
        hull_ms = median_events(lambda: spheres_init.visual_hull(target, mvp, grid=grid), args.reps)
        hull = spheres_init.visual_hull(target, mvp, grid=grid)
        edt = median_events(lambda: spheres_init._edt(hull), args.reps)
        d2 = spheres_init.distance_transform_sq(hull)
        cover = median_events(lambda: spheres_init._cover(hull, d2, args.spheres, -1.0, 1.0, 0.05, 0.92), args.reps)
        row["device"]["stages_ms"] = {"pack": pack, "carve": hull_ms - pack, "edt": edt, "cover": cover,
                                      "note": "pack = the hull call on one voxel outside every frustum; carve = the hull call minus pack; buffers allocated inside each call"}
        try:
            t, all_t, out = median_wall(lambda: train_object.place_spheres(target, mvp, args.spheres, grid=grid), args.reps)
            centres, radii, hull_frac, left = out
            row["host"] = {"ms": 1e3 * t, "ms_all": [1e3 * x for x in all_t], "spheres": int(len(radii)), "hull_fraction": hull_frac, "uncovered_fraction": left,
                           "radii_min_max": [float(radii.min()), float(radii.max())] if len(radii) else None}
            row["host"]["same_centres_as_device"] = bool(len(radii) == len(kp) and np.array_equal(centres, kp.pt))
            row["host"]["max_abs_radius_difference"] = float(np.abs(radii - kp.r).max()) if len(radii) == len(kp) and len(kp) else None
            row["host_over_device"] = row["host"]["ms"] / row["device"]["ms"]
        except (MemoryError, torch.cuda.OutOfMemoryError) as exc:
            row["host"] = {"did_not_fit": f"{type(exc).__name__}: {exc}"[:200]}
        rec["grids"][str(grid)] = row
        print(f"grid {grid}: {json.dumps(row)}", file=sys.stderr, flush=True)
    first = rec["grids"].get("72") or next(iter(rec["grids"].values()))
    rec["value"] = first.get("host_over_device")

    if not args.no_train:
        fits = {}
        for placement in ("host", "device"):
            r = train_object.run(n_spheres=args.spheres, k=args.k, views=args.views, res=args.res, iters=args.iters, stages=False, placement=placement)
            fits[placement] = {"spheres_placed": r["spheres"]["placed"], "silhouette_iou": r["silhouette_iou"], "silhouette_iou_at_start": r["silhouette_iou_at_start"],
                               "inverted_tets": r["inverted_tets"], "ms_per_iteration": r["ms_per_iteration"]}
        recorded = None
        try:
            recorded = json.load(open(os.path.join(ROOT, "profiles", "r06_train_mario.json")))["silhouette_iou"]
        except (OSError, KeyError, ValueError):
            pass
        rec["train_object"] = {"iterations": args.iters, "host": fits["host"], "device": fits["device"],
                               "same_sphere_count": fits["host"]["spheres_placed"] == fits["device"]["spheres_placed"],
                               "iou_difference": abs(fits["host"]["silhouette_iou"] - fits["device"]["silhouette_iou"]),
                               "recorded_iou_r06_train_mario": recorded}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: rec[k] for k in ("metric", "value", "unit") if k in rec} | {"train_object": rec.get("train_object"),
                      "grids": {g: {"device_ms": r["device"]["ms"], "host_ms": r.get("host", {}).get("ms")} for g, r in rec["grids"].items()}}))


if __name__ == "__main__":
    main()
