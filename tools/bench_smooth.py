#!/usr/bin/env python3
"""The surface smoother, timed: `smooth.adjacency`, 10 Taubin and 10 tangential iterations in both state layouts, and the projection, on the
mario target mesh and the mario scene merged at grid 128 and 256.

    python tools/bench_smooth.py [--reps 7 --grids 128 256 --iterations 10 --out profiles/smooth_bench.json]

Timing: HIP events around each call after one warm-up, medians of --reps with their minimum and maximum; run it in a fresh process.
`taubin_ms` / `tangential_ms` are the iterations alone (`smooth._run`: the float64 state made of `v`, then `tsamd_smooth_run`), once per
state layout -- records of 4 float64 (32 bytes, never across a 128-byte line) and of 3 (24 bytes, one in eight straddles); the two must
give the same bytes.  `smooth_call_ms` is the whole `smooth.smooth` with the adjacency handed in (classification, iterations, the
final cast and the readback of the counts); `project_ms` is the `metrics.nearest_on_mesh` of the smoothed vertices on the input.

The baseline is the same arithmetic in plain torch on the same GPU: `index_add_` of the float64 neighbours over the adjacency's pairs,
a division, and for the tangential mode `torch.cross` per face and three more `index_add_`.  Its sums come from float atomics, so it is
not bitwise repeatable; it must agree with the device to 1e-12 of the mesh's extent.

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


def torch_smooth(v, faces, adj, cls, iterations, mode, lam, mu):
    """The baseline: the float64 state after `iterations` iterations."""
    import torch
    Nv = int(v.shape[0])
    deg = (adj.offsets[1:] - adj.offsets[:-1]).long()
    row = torch.repeat_interleave(torch.arange(Nv, device=v.device), deg)
    nb = adj.neighbours.long()
    degf = deg.double()[:, None]
    move = (cls == 0)[:, None]
    f = faces[adj.valid != 0].long()
    p = v.double()
    for _ in range(iterations):
        for c in ((lam, mu) if mode == "taubin" else (lam,)):
            if c == 0.0:
                continue
            L = torch.zeros_like(p).index_add_(0, row, p[nb]) / degf - p
            d = c * L
            if mode == "taubin":
                q = p + d
            else:
                a = p[f[:, 0]]
                N = torch.cross(p[f[:, 1]] - a, p[f[:, 2]] - a, dim=1)
                n = torch.zeros_like(p).index_add_(0, f[:, 0], N).index_add_(0, f[:, 1], N).index_add_(0, f[:, 2], N)
                nn = (n * n).sum(1, keepdim=True)
                q = torch.where(nn > 0, p + (d - n * ((d * n).sum(1, keepdim=True) / nn)), p)
            p = torch.where(move, q, p)
    return p


def smooth_kernels(lib):
    """kernel -> registers, scratch and LDS, from the code object's metadata."""
    import re
    import kernel_metadata
    out = {}
    for k, v in kernel_metadata.kernel_metadata(lib).items():
        m = re.search(r"smooth_[a-z]+_kernel(<[^>]*>)?", k)
        if m:
            out[m.group(0)] = {"vgpr_count": v["vgpr_count"], "sgpr_count": v["sgpr_count"], "scratch_bytes": v["private_segment_fixed_size"],
                               "lds_bytes": v["group_segment_fixed_size"]}
    return out


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def bench_mesh(name, v, f, args):
    import torch
    from tssplat_amd import metrics, quality, smooth
    Nv, Nt, it = int(v.shape[0]), int(f.shape[0]), args.iterations
    adj_ms, adj_span, adj = median_events(lambda: smooth.adjacency(f, Nv), args.reps)
    mesh = smooth._mesh_struct(adj, f, Nv)
    cls = smooth._classify(v, mesh, adj, None, "fixed")
    deg = (adj.offsets[1:] - adj.offsets[:-1])
    extent = float((v[torch.isfinite(v).all(1)].max() - v[torch.isfinite(v).all(1)].min()))
    rec = {"vertices": Nv, "triangles": Nt, "iterations": it, "adjacency_ms": adj_ms, "adjacency_ms_min_max": adj_span, "neighbour_entries": int(adj.neighbours.shape[0]),
           "degree_max": int(deg.max()), "degree_mean": float(deg.double().mean()), "irregular_vertices": int(adj.irregular.sum()), "valid_faces": int(adj.valid.sum()),
           "moved": int((cls == 0).sum()), "extent": extent}
    for mode in smooth.MODES:
        states = {}
        for stride in (4, 3):
            ms, span, state = median_events(lambda: smooth._run(v, mesh, cls, it, mode, 0.5, -0.53, None, stride), args.reps)
            states[stride] = state
            rec[f"{mode}_ms_stride{stride}"], rec[f"{mode}_ms_stride{stride}_min_max"] = ms, span
        assert torch.equal(states[3].contiguous().view(torch.int64), states[4].contiguous().view(torch.int64)), f"{name} {mode}: the two layouts disagree"
        base_ms, base_span, base = median_events(lambda: torch_smooth(v, f, adj, cls, it, mode, 0.5, -0.53), args.baseline_reps)
        err = float((base - states[4]).abs().max()) / extent
        assert err <= 1e-12, f"{name} {mode}: the torch statement is {err:.3e} of the extent away"
        best = min(rec[f"{mode}_ms_stride4"], rec[f"{mode}_ms_stride3"])
        used = rec[f"{mode}_ms_stride{smooth.STATE_STRIDE}"]
        rec.update({f"{mode}_ms": used, f"{mode}_ms_min_max": rec[f"{mode}_ms_stride{smooth.STATE_STRIDE}_min_max"], f"{mode}_state_sha256": sha(states[4]),
                    f"{mode}_stride3_over_stride4": rec[f"{mode}_ms_stride3"] / rec[f"{mode}_ms_stride4"],
                    f"{mode}_torch_ms": base_ms, f"{mode}_torch_ms_min_max": base_span, f"{mode}_torch_max_error_over_extent": err, f"{mode}_torch_over_device": base_ms / used,
                    f"{mode}_device_faster_than_torch_beyond_spread": base_span[0] > rec[f"{mode}_ms_stride{smooth.STATE_STRIDE}_min_max"][1],
                    f"{mode}_best_layout_ms": best})
        call_ms, call_span, out = median_events(lambda: smooth.smooth(v, f, iterations=it, mode=mode, adjacency=adj), args.reps)
        rec[f"{mode}_smooth_call_ms"], rec[f"{mode}_smooth_call_ms_min_max"] = call_ms, call_span
        assert torch.equal(out.v.view(torch.int32), torch.where((cls == 0)[:, None], states[4].float(), v).view(torch.int32)), f"{name} {mode}: smooth() and _run disagree"
        sh = quality.shape(out.v, f)
        rec[f"{mode}_shape_after"] = {"alr_mean": sh.alr_mean, "alr_p05": sh.alr_p05, "alr_min": sh.alr_min, "min_angle_min": sh.min_angle_min}
        if mode == "tangential":
            proj_ms, proj_span, proj = median_events(lambda: metrics.nearest_on_mesh(out.v, v, f), args.reps)
            rec["project_ms"], rec["project_ms_min_max"] = proj_ms, proj_span
            rec["project_max_d2_before"] = float(proj[0].max())
    sh = quality.shape(v, f)
    rec["shape_before"] = {"alr_mean": sh.alr_mean, "alr_p05": sh.alr_p05, "alr_min": sh.alr_min, "min_angle_min": sh.min_angle_min}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--baseline-reps", type=int, default=7)
    ap.add_argument("--grids", type=int, nargs="*", default=[128, 256])
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_bench.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import train_object
    import tssplat_amd.dr as dr
    from tssplat_amd import _capi, geometry, merge, scenes, smooth, spheres_init

    assert torch.cuda.is_available(), "bench_smooth.py needs a GPU"
    tgt = np.load(os.path.join(ROOT, "tests", "golden", "mario_mesh.npz"))
    tv = torch.from_numpy(tgt["vertices"].astype(np.float32)).cuda()
    tf = torch.from_numpy(tgt["faces"].astype(np.int32)).cuda()
    mvp = torch.from_numpy(scenes.dataset_mvps(120)).cuda()
    with torch.no_grad():
        target = train_object.render_alpha(dr.RasterizeCudaContext(), tv, tf, mvp, 512).clone()
    kp = spheres_init.init_spheres(target, mvp, 20, grid=72)
    geo = geometry.TetMeshMultiSphereGeometry(kp, k=8)
    try:
        kernels = smooth_kernels(_capi.lib_path())
    except Exception as exc:                                              # the LLVM tools are not there
        kernels = {"unavailable": repr(exc)}
    rec = {"metric": f"{args.iterations} Taubin iterations on the largest mesh, plain torch over the device", "unit": "x", "higher_is_better": True,
           "config": {"timing": f"HIP events around each call after one warm-up; medians of {args.reps} calls ({args.baseline_reps} for the torch statement), one process",
                      "state_stride": smooth.STATE_STRIDE, "lam": 0.5, "mu": -0.53, "boundary": "fixed", "kernels": kernels,
                      "workload": f"mario fixture: the target mesh; {len(kp)} initial tet-spheres x kuhn8 merged at grids {args.grids}"},
           "meshes": {}}
    meshes = [("mario_target", tv, tf)]
    for g in args.grids:
        m = merge.merge_tets(geo.tet_v.detach().contiguous(), geo.tet_elem, grid=g)
        meshes.append((f"merged_grid_{g}", m.v.contiguous(), m.faces.contiguous()))
    keys = ("vertices", "adjacency_ms", "taubin_ms", "taubin_ms_stride3", "taubin_torch_over_device", "tangential_ms", "tangential_ms_stride3",
            "tangential_torch_over_device", "project_ms")
    for name, v, f in meshes:
        rec["meshes"][name] = bench_mesh(name, v, f, args)
        print(name, json.dumps({k: rec["meshes"][name][k] for k in keys}), file=sys.stderr, flush=True)
    last = rec["meshes"][meshes[-1][0]]
    rec["value"] = last["taubin_torch_over_device"]
    rec["device_faster_than_torch_beyond_spread_on_the_largest_mesh"] = last["taubin_device_faster_than_torch_beyond_spread"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"metric": rec["metric"], "value": rec["value"], "unit": "x", "meshes": {k: {x: m[x] for x in keys} for k, m in rec["meshes"].items()}}))


if __name__ == "__main__":
    main()
