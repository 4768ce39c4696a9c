#!/usr/bin/env python
"""Timings of the mesh voxeliser (tssplat_amd.voxelize) on one GPU, against a plain-torch statement of the same integers.

Meshes: `target`, the mario fixture's mesh (7 409 triangles, a few columns each at these grids), and `merged`, the fixture's 20 x kuhn8
tet-spheres as `spheres_init.init_spheres` places them, merged at grid 256 (tools/bench_simplify.py's workload: sub-cell triangles).
Each is voxelised at --grids nodes per axis over `merge.default_bounds` of its vertices: `winding` along every axis and
`occupancy(rays=3)`.  Median of --reps runs after one warm-up, HIP events around the call, its one readback included.

Baseline: `torch_winding` below -- the lattice, the int64 edge functions and fill rule and the float64 crossing of tests/voxel_oracle.py
in plain torch ops: the (face, candidate column) pairs expanded with `repeat_interleave`, `index_add_` on int32, `cumsum`.  Its `w` must
equal the kernels' bit for bit (asserted).  `torch_occupancy` is three of them, the rule and the vote.

Per row the time is also set against the bytes the call cannot avoid -- the deposit slabs cleared and read once, (G + 1) G^2 x 4 B each per
ray, and the output written (the occupancy byte: written by three passes and read by two) -- over the copy ceiling BASELINE.md's
roofline uses (6.29 TB/s).

    python tools/bench_voxelize.py [--grids 128 256 --reps 5 --out profiles/voxelize_bench.json]

One JSON line on stdout; the whole record goes to --out."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

COPY_CEILING_TB_S = 6.29
S_BITS = 10
S = 1 << S_BITS


def torch_winding(v, faces, G, lo, hi, axis):
    """int32 [G, G, G]: tests/voxel_oracle.py's `winding` in plain torch on the device (valid, finite meshes inside 2^19 nodes only)."""
    import torch
    b, c = (axis + 1) % 3, (axis + 2) % 3
    h = (hi - lo) / G
    t = (v.double() - lo) / h
    u = torch.floor(t * float(S) + 0.5).long()
    r = t - 0.5
    f = faces.long()
    A, B, C = u[f[:, 0]], u[f[:, 1]], u[f[:, 2]]
    Ab, Ac, Bb, Bc, Cb, Cc = A[:, b], A[:, c], B[:, b], B[:, c], C[:, b], C[:, c]
    area = (Bb - Ab) * (Cc - Ac) - (Bc - Ac) * (Cb - Ab)
    b0 = torch.clamp((torch.minimum(torch.minimum(Ab, Bb), Cb) + (S // 2 - 1)) >> S_BITS, min=0)
    b1 = torch.clamp((torch.maximum(torch.maximum(Ab, Bb), Cb) - S // 2) >> S_BITS, max=G - 1)
    c0 = torch.clamp((torch.minimum(torch.minimum(Ac, Bc), Cc) + (S // 2 - 1)) >> S_BITS, min=0)
    c1 = torch.clamp((torch.maximum(torch.maximum(Ac, Bc), Cc) - S // 2) >> S_BITS, max=G - 1)
    nc = torch.clamp(c1 - c0 + 1, min=0)
    cols = torch.clamp(b1 - b0 + 1, min=0) * nc * (area != 0)
    fi = torch.repeat_interleave(torch.arange(f.shape[0], device=v.device), cols)
    start = torch.cumsum(cols, 0) - cols
    local = torch.arange(fi.shape[0], device=v.device) - start[fi]
    ncf = nc[fi]
    p, q = b0[fi] + local // ncf, c0[fi] + local % ncf
    Pb, Pc = p * S + S // 2, q * S + S // 2
    Ab, Ac, Bb, Bc, Cb, Cc, ar = Ab[fi], Ac[fi], Bb[fi], Bc[fi], Cb[fi], Cc[fi], area[fi]
    sg = torch.sign(ar)

    def edge(Qb, Qc, Rb, Rc):
        E = (Rb - Qb) * (Pc - Qc) - (Rc - Qc) * (Pb - Qb)
        e, db, dc = sg * E, sg * (Rb - Qb), sg * (Rc - Qc)
        return E, (e > 0) | ((e == 0) & ((db > 0) | ((db == 0) & (dc > 0))))

    (E_BC, in_bc), (E_CA, in_ca), (E_AB, in_ab) = edge(Bb, Bc, Cb, Cc), edge(Cb, Cc, Ab, Ac), edge(Ab, Ac, Bb, Bc)
    cover = in_bc & in_ca & in_ab
    ra, rb, rc = r[f[fi, 0], axis], r[f[fi, 1], axis], r[f[fi, 2], axis]
    x = ((E_BC.double() * ra + E_CA.double() * rb) + E_AB.double() * rc) / ar.double()
    i0 = torch.clamp(torch.ceil(x), 0.0, float(G)).long()
    dep = torch.zeros((G + 1) * G * G, dtype=torch.int32, device=v.device)
    dep.index_add_(0, ((i0 * G + p) * G + q)[cover], (-sg[cover]).int())
    w = torch.cumsum(dep.reshape(G + 1, G, G), 0, dtype=torch.int32)[:G]
    order = (axis, b, c)
    return w.permute([order.index(world) for world in range(3)]).contiguous()


def torch_occupancy(v, faces, G, lo, hi):
    bits = [torch_winding(v, faces, G, lo, hi, axis) != 0 for axis in range(3)]
    return (bits[0].int() + bits[1].int() + bits[2].int()) >= 2


def merged_mario(grid, views=120, res=512, spheres=20, k=8):
    """(v, faces) of tools/bench_simplify.py's workload and the fixture's own mesh."""
    import numpy as np
    import torch
    import train_object
    import tssplat_amd.dr as dr
    from tssplat_amd import geometry, merge, scenes, spheres_init
    tgt = np.load(os.path.join(ROOT, "tests", "golden", "mario_mesh.npz"))
    tv = torch.from_numpy(tgt["vertices"].astype(np.float32)).cuda()
    tf = torch.from_numpy(tgt["faces"].astype(np.int32)).cuda()
    mvp = torch.from_numpy(scenes.dataset_mvps(views)).cuda()
    with torch.no_grad():
        target = train_object.render_alpha(dr.RasterizeCudaContext(), tv, tf, mvp, res).clone()
    kp = spheres_init.init_spheres(target, mvp, spheres, grid=72)
    geo = geometry.TetMeshMultiSphereGeometry(kp, k=k)
    merged = merge.merge_tets(geo.tet_v.detach().contiguous(), geo.tet_elem, grid=grid)
    return (tv, tf), (merged.v, merged.faces)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--merge-grid", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxelize_bench.json"))
    args = ap.parse_args()

    import torch
    from bench_merge import median_events
    from tssplat_amd import merge, voxelize

    assert torch.cuda.is_available(), "bench_voxelize.py needs a GPU"
    target, merged = merged_mario(args.merge_grid)
    rec = {"metric": "mesh voxelisation (integer winding number on the merge's grid), ms per call", "unit": "ms", "higher_is_better": False,
           "config": {"meshes": {"target": f"mario fixture: {int(target[1].shape[0])} triangles",
                                 "merged": f"merge_tets of the fixture's tet-spheres at grid {args.merge_grid}: {int(merged[1].shape[0])} triangles"},
                      "timing": f"median of {args.reps} runs after one warm-up; HIP events around the call, its readback included",
                      "baseline": "torch_winding / torch_occupancy of this tool: (face x candidate column) expansion, index_add_ on int32, cumsum; w asserted equal",
                      "copy_ceiling_TB_per_s": COPY_CEILING_TB_S,
                      "floor_bytes": "per ray (G + 1) G^2 x 4 B cleared and the same read; winding: + G^3 x 4 B written; occupancy(rays=3): + G^3 x 1 B written three times and read twice"},
           "rows": [], "kernel_slower_than_baseline": []}
    for name, (v, f) in (("target", target), ("merged", merged)):
        for G in args.grids:
            lo, hi = merge.default_bounds(v, G)
            slab = (G + 1) * G * G * 4
            for axis in range(3):
                ms, got = median_events(lambda: voxelize.winding(v, f, G, (lo, hi), axis), args.reps)
                base_ms, want = median_events(lambda: (torch_winding(v, f, G, lo, hi, axis), torch.cuda.synchronize())[0], args.reps)
                assert torch.equal(got.w, want), (name, G, axis)
                floor = 2 * slab + G ** 3 * 4
                rec["rows"].append({"mesh": name, "grid": G, "call": f"winding(axis={axis})", "ms": ms, "torch_ms": base_ms, "torch_over_kernel": base_ms / ms,
                                    "floor_bytes": floor, "share_of_copy_ceiling": floor / (ms * 1e-3) / (COPY_CEILING_TB_S * 1e12), "w_equal_bitwise": True,
                                    "open_columns": got.open_columns, "deposits": got.deposits, "wave_faces": got.wave_faces, "degenerate_faces": got.degenerate_faces})
            ms, got = median_events(lambda: voxelize.occupancy(v, f, G, (lo, hi)), args.reps)
            base_ms, want = median_events(lambda: (torch_occupancy(v, f, G, lo, hi), torch.cuda.synchronize())[0], args.reps)
            assert torch.equal(got.occ, want), (name, G)
            floor = 3 * 2 * slab + 5 * G ** 3
            rec["rows"].append({"mesh": name, "grid": G, "call": "occupancy(rays=3)", "ms": ms, "torch_ms": base_ms, "torch_over_kernel": base_ms / ms,
                                "floor_bytes": floor, "share_of_copy_ceiling": floor / (ms * 1e-3) / (COPY_CEILING_TB_S * 1e12), "occ_equal_bitwise": True,
                                "open_columns": list(got.open_columns), "disputed": got.disputed, "inside": int(got.occ.sum()), "deposits": list(got.deposits),
                                "wave_faces": got.wave_faces})
            for row in rec["rows"][-4:]:
                print(json.dumps(row), file=sys.stderr, flush=True)
    rec["kernel_slower_than_baseline"] = [f"{r['mesh']} {r['grid']} {r['call']}" for r in rec["rows"] if r["torch_over_kernel"] < 1.0]
    head = [r for r in rec["rows"] if r["mesh"] == "merged" and r["grid"] == max(args.grids) and r["call"].startswith("occupancy")][0]
    rec["value"] = head["ms"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"metric": rec["metric"], "value": rec["value"], "unit": "ms", "mesh": "merged", "grid": head["grid"], "call": head["call"],
                      "torch_over_kernel": head["torch_over_kernel"], "share_of_copy_ceiling": head["share_of_copy_ceiling"],
                      "kernel_slower_than_baseline": rec["kernel_slower_than_baseline"]}))


if __name__ == "__main__":
    main()
