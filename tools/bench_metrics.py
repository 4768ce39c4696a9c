#!/usr/bin/env python3
"""The surface metrics, timed: `metrics.sample_surface`, `metrics.nearest` and `metrics.compare`, and one `compare_meshes` of the
grid-256 merged mario scene against its target mesh.

    python tools/bench_metrics.py [--sizes 10000 100000 200000 --reps 7 --baseline-reps 3 --out profiles/metrics_bench.json]
                                  [--variants nearest_q2 nearest_q8 nearest_tile256 nearest_tile4096 nearest_minscan]
    python tools/bench_metrics.py --exact [--exact-variants pointmesh_count pointmesh_noprune pointmesh_q2 pointmesh_q4 pointmesh_tile256]

`nearest` runs at N = M in --sizes on normally distributed points (no ties, no NaN).  The baseline is plain torch on the same GPU:
the same float32 form `((qx - rx)^2 + (qy - ry)^2) + (qz - rz)^2`, broadcast over a block of queries at a time so that the N x block
distance matrix fits, then `min` over the ref axis; the bench asserts that both give the same `idx`.  Timing: HIP events around each
call after a warm-up, medians.  Next to the times the record holds the pairs per second, the VALU instructions per pair counted in the
kernel's ISA (the path every trip of the inner loop takes; its LDS reads times the queries per lane are its pairs) and the share of the FP32 vector issue rate that makes.  157.3 TFLOPS is 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz with a fused
multiply-add counted as two: 78.6 T lane-operations per second for instructions that are not packed.  (Half of that, 39.3 T, is what a
rate that already counted packed pairs would leave; the record keeps the share against it too -- a share above 1 rules it out.)

The scene of the last part is tools/bench_merge.py's: the mario fixture's initial 20 x kuhn8 tet-spheres merged at 256 nodes per axis.

--variants: the kernel's levers, priced once each.  Every name is a laboratory build of tools/lab_variants.py (built beforehand:
`python tools/lab_variants.py NAME ...`); each runs `nearest` at N = M = 100 000 in a fresh child process under TSSPLAT_AMD_LIB, the product
library in between, every one with the chunk count that gives its workgroup size about 1 024 workgroups, and is held to the torch
baseline's `idx` like the product.  The record gains `levers`.

--exact: the point-to-triangle search instead (`metrics.nearest_on_mesh`, `metrics.compare_meshes_exact`), on the same scene: --samples samples
of the merged surface against the target mesh and of the target against the merged surface, each beside a plain-torch float64 chunked
statement of the same formula that must give the same `tri` and `d2` (against the merged surface on the first --baseline-queries queries,
the time scaled to all of them and said so); the share of pairs that reach the float64 evaluation (laboratory build `pointmesh_count`) and the
levers of --exact-variants, `pointmesh_noprune` among them, each in a fresh child process with the product in between and held to the
SHA-256 of the product's `tri` and `d2` bytes, with the registers of its kernels from the code object's metadata;
`compare_meshes_exact` beside `compare_meshes`, for the merged surface against the target and for the k = 4 simplified surface against
the unsimplified one.  The record is APPENDED to the list in --exact-out (profiles/metrics_exact_bench.json).

One JSON line on stdout; the whole record goes to --out."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

PEAK_LANE_OPS = 157.3e12 / 2       # FP32 vector: 2 flops per FMA, one instruction per lane and clock counted once


def median_events(fn, reps):
    """(median milliseconds between two HIP events around `fn`, [min, max], last result): `reps` calls after one warm-up."""
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
    return statistics.median(times), [min(times), max(times)], out


def torch_nearest(query, ref, budget_bytes=1 << 30):
    """The baseline: chunked broadcast in plain torch, the same float32 form."""
    import torch
    rows = max(1, budget_bytes // (4 * int(ref.shape[0])))
    rx, ry, rz = (ref[:, k][None, :] for k in range(3))
    d2_out, idx_out = [], []
    for s in range(0, int(query.shape[0]), rows):
        c = query[s:s + rows]
        dx, dy, dz = c[:, 0:1] - rx, c[:, 1:2] - ry, c[:, 2:3] - rz
        d2, idx = torch.min((dx * dx + dy * dy) + dz * dz, dim=1)
        d2_out.append(d2)
        idx_out.append(idx)
    return torch.cat(d2_out), torch.cat(idx_out).int()


def hot_loop(lib, queries_per_lane):
    """Counted in the disassembly of nearest_points_kernel: the path every trip of the inner loop takes.  The loop's head is the target of
    the backward branches behind the LDS reads; the walk goes from there in address order, jumps over what a forward `s_cbranch_execz`
    skips when no lane takes it (the scan for the index where the group minimum improves: rare once the stream is a few thousand points
    old) and ends at the first branch back to the head."""
    import re
    import tempfile
    import kernel_metadata
    want = "nearest_points_kernel"
    ins = []                                                  # (offset in the kernel, mnemonic, branch target offset or None)
    with tempfile.TemporaryDirectory() as d:
        for co in kernel_metadata._code_objects(lib, d):
            text = subprocess.check_output([os.path.join(kernel_metadata.LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], text=True)
            if want not in text:
                continue
            inside = False
            for ln in text.split("\n"):
                m = re.match(r"^([0-9a-f]+) <(\S+)>:$", ln)
                if m:
                    inside, start, name = want in m.group(2), int(m.group(1), 16), m.group(2)
                    continue
                m = re.match(r"^\s+(\S+).*//\s*([0-9A-F]+):", ln)
                if inside and m:
                    t = re.search(r"<\S+\+0x([0-9a-f]+)>\s*$", ln)
                    ins.append((int(m.group(2), 16) - start, m.group(1), int(t.group(1), 16) if t and m.group(1).startswith(("s_cbranch", "s_branch")) else None))
                if inside and ln.strip().startswith("s_endpgm"):
                    inside = False
    first_read = next(o for o, op, _ in ins if op.startswith("ds_read"))
    head = max(t for o, op, t in ins if t is not None and t <= first_read and o > first_read)
    valu = reads = packed = total = 0
    skip_to = None
    for o, op, t in ins:
        if o < head or (skip_to is not None and o < skip_to):
            continue
        total += 1
        valu += op.startswith("v_")
        packed += op.startswith("v_pk_")
        reads += op.startswith("ds_read")
        if t == head:
            break
        if op == "s_cbranch_execz" and t is not None and t > o:
            skip_to = t
    meta = {k: v for k, v in kernel_metadata.kernel_metadata(lib).items() if want in k}
    (name, meta), = meta.items()
    return {"kernel": name, "instructions": total, "valu": valu, "packed_valu": packed, "lds_reads": reads, "pairs": reads * queries_per_lane,
            "valu_per_pair": valu / (reads * queries_per_lane), "vgpr_count": meta["vgpr_count"], "scratch_bytes": meta["private_segment_fixed_size"],
            "lds_bytes": meta["group_segment_fixed_size"]}


def torch_nearest_on_mesh(query, v, faces, budget_bytes=1 << 28):
    """The baseline of --exact: tests/pointmesh_oracle.py's statement in plain float64 torch, a block of queries against all triangles at a
    time; the minimum is taken on bits(fl32 d2) << 32 | triangle, like the kernel's.  Returns (d2 float32, tri int32)."""
    import torch
    T = int(faces.shape[0])
    f = faces.long()
    ok = ((f >= 0) & (f < v.shape[0])).all(dim=1)
    p = v.double()[f.clamp(0, max(int(v.shape[0]) - 1, 0))]
    A, B, C = p[:, 0], p[:, 1], p[:, 2]
    AB, AC = B - A, C - A
    n = torch.stack([AB[:, 1] * AC[:, 2] - AB[:, 2] * AC[:, 1], AB[:, 2] * AC[:, 0] - AB[:, 0] * AC[:, 2], AB[:, 0] * AC[:, 1] - AB[:, 1] * AC[:, 0]], dim=1)
    ok &= torch.isfinite(p).all(dim=2).all(dim=1) & (torch.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]) > 0)
    ids = torch.arange(T, device=v.device, dtype=torch.int64)[None, :]
    none = torch.full((), 2 ** 63 - 1, dtype=torch.int64, device=v.device)

    def dot(u, w):
        return (u[..., 0] * w[..., 0] + u[..., 1] * w[..., 1]) + u[..., 2] * w[..., 2]
    rows = max(1, budget_bytes // (8 * 3 * T))
    d2_out, tri_out = [], []
    for s0 in range(0, int(query.shape[0]), rows):
        P = query[s0:s0 + rows].double()[:, None, :]
        AP, BP, CP = P - A, P - B, P - C
        d1, d2, d3, d4, d5, d6 = dot(AB, AP), dot(AC, AP), dot(AB, BP), dot(AC, BP), dot(AB, CP), dot(AC, CP)
        del AP, BP, CP
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e, g = d4 - d3, d5 - d6
        s = (va + vb) + vc
        vv, ww = vb / s, vc / s                                            # interior, then every other region over it, the first test last
        w_bc = e / (e + g)
        zero, one = torch.zeros_like(d1), torch.ones_like(d1)
        for test, v_r, w_r in [((va <= 0) & (e >= 0) & (g >= 0), one - w_bc, w_bc), ((vb <= 0) & (d2 >= 0) & (d6 <= 0), zero, d2 / (d2 - d6)),
                               ((d6 >= 0) & (d5 <= d6), zero, one), ((vc <= 0) & (d1 >= 0) & (d3 <= 0), d1 / (d1 - d3), zero),
                               ((d3 >= 0) & (d4 <= d3), one, zero), ((d1 <= 0) & (d2 <= 0), zero, zero)]:
            vv, ww = torch.where(test, v_r, vv), torch.where(test, w_r, ww)
        del d1, d2, d3, d4, d5, d6, vc, vb, va, e, g, s, w_bc
        D = P - ((A + AB * vv[..., None]) + AC * ww[..., None])
        dist2 = ((D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1]) + D[..., 2] * D[..., 2])
        key = (dist2.float().view(torch.int32).long() << 32) | ids
        key = torch.where(ok[None, :] & ~torch.isnan(dist2), key, none).min(dim=1).values
        d2_out.append(torch.where(key == none, torch.full_like(key, 0x7F800000), key >> 32).int().view(torch.float32))
        tri_out.append(torch.where(key == none, torch.full_like(key, -1), key & 0xFFFFFFFF).int())
    return torch.cat(d2_out), torch.cat(tri_out)


def digests(d2, tri):
    """SHA-256 of the bytes of both results: what a laboratory build is held to the product by."""
    import hashlib
    return {"d2_sha256": hashlib.sha256(d2.cpu().numpy().tobytes()).hexdigest(), "tri_sha256": hashlib.sha256(tri.cpu().numpy().tobytes()).hexdigest()}


def pointmesh_kernels(lib):
    """kernel -> registers, scratch and LDS, from the code object's metadata."""
    import kernel_metadata
    return {k.split("pointmesh_")[1].split("_kernel")[0]: {"vgpr_count": v["vgpr_count"], "sgpr_count": v["sgpr_count"], "scratch_bytes": v["private_segment_fixed_size"],
                                                           "lds_bytes": v["group_segment_fixed_size"]}
            for k, v in kernel_metadata.kernel_metadata(lib).items() if "pointmesh_" in k}


def exact_bench(args):
    """--exact (and, with --exact-child, one timing of it under whatever library TSSPLAT_AMD_LIB names)."""
    import numpy as np
    import torch
    import train_object
    import tssplat_amd.dr as dr
    from tssplat_amd import _capi, geometry, merge, metrics, scenes, simplify, spheres_init

    tgt = np.load(os.path.join(ROOT, "tests", "golden", "mario_mesh.npz"))
    tv = torch.from_numpy(tgt["vertices"].astype(np.float32)).cuda()
    tf = torch.from_numpy(tgt["faces"].astype(np.int32)).cuda()
    mvp = torch.from_numpy(scenes.dataset_mvps(120)).cuda()
    with torch.no_grad():
        target = train_object.render_alpha(dr.RasterizeCudaContext(), tv, tf, mvp, 512).clone()
    kp = spheres_init.init_spheres(target, mvp, 20, grid=72)
    geo = geometry.TetMeshMultiSphereGeometry(kp, k=8)
    merged = merge.merge_tets(geo.tet_v.detach().contiguous(), geo.tet_elem, grid=args.grid)
    n = args.samples
    sa, sb = metrics.sample_surface(merged.v, merged.faces, n, 2), metrics.sample_surface(tv, tf, n, 0)
    sides = {"merged_samples_against_target": (sa.points, tv, tf), "target_samples_against_merged": (sb.points, merged.v, merged.faces)}
    info = metrics.nearest_on_mesh_info(1, 1)
    if args.exact_child:
        out = {}
        for key, (q, v, f) in sides.items():
            ms, span, (d2, tri, _) = median_events(lambda: metrics.nearest_on_mesh(q, v, f, ref_chunks=args.ref_chunks, return_points=False), args.reps)
            out[key] = {"ms": ms, "ms_min_max": span, "tri_sum": int(tri.long().sum()), **digests(d2, tri)}
        print(json.dumps(out))
        return
    rec = {"metric": "compare_meshes_exact on the grid-%d merged mario against its target, %d samples per surface" % (args.grid, n), "unit": "ms", "higher_is_better": False,
           "config": {"timing": f"HIP events around each call after one warm-up; medians of {args.reps} calls ({args.baseline_reps} for the torch baseline)",
                      "block": info.block, "queries_per_lane": info.queries_per_lane, "tri_tile": info.tri_tile, "kernels": pointmesh_kernels(_capi.lib_path()),
                      "workload": f"mario fixture, {len(kp)} initial tet-spheres x kuhn8 merged at grid {args.grid}: {int(merged.faces.shape[0])} triangles; the target mesh: "
                                  f"{int(tf.shape[0])} triangles; {n} samples per surface"},
           "nearest_on_mesh": {}}
    for key, (q, v, f) in sides.items():
        T = int(f.shape[0])
        ms, span, (d2, tri, _) = median_events(lambda: metrics.nearest_on_mesh(q, v, f), args.reps)
        nb = n if T * n <= 2 * 10 ** 9 else min(n, args.baseline_queries)
        base_ms, base_span, (bd2, btri) = median_events(lambda: torch_nearest_on_mesh(q[:nb], v, f), args.baseline_reps)
        assert torch.equal(tri[:nb], btri), f"{key}: the kernel and the torch baseline disagree on {int((tri[:nb] != btri).sum())} triangles"
        assert torch.equal(d2[:nb].view(torch.int32), bd2.view(torch.int32)), f"{key}: the kernel and the torch baseline disagree on d2"
        rec["nearest_on_mesh"][key] = {"queries": n, "triangles": T, "kernel_ms": ms, "kernel_ms_min_max": span, "pairs_per_s": float(n) * T / (ms * 1e-3),
                                       "auto_chunks": metrics.nearest_on_mesh_info(n, T).auto_chunks, "torch_float64_queries": nb, "torch_float64_ms": base_ms,
                                       "torch_float64_ms_min_max": base_span, "torch_float64_ms_scaled_to_all_queries": base_ms * n / nb,
                                       "torch_over_kernel": base_ms * n / nb / ms, "tri_and_d2_identical": True,
                                       "mean_d": float(torch.sqrt(d2).double().mean()), **digests(d2, tri)}
    if args.exact_variants:
        import lab_variants
        levers = {}
        for name in ["product"] + [x for v in args.exact_variants for x in (v, "product")]:
            per_lane = int(name[len("pointmesh_q"):]) if name.startswith("pointmesh_q") else info.queries_per_lane
            chunks = 0 if per_lane == info.queries_per_lane else -(-1024 // -(-n // (info.block * per_lane)))
            env = dict(os.environ)
            if name != "product":
                env["TSSPLAT_AMD_LIB"] = os.path.join(ROOT, "tssplat_amd", f"libtssplat_amd_{name}.so")
            reps = 1 if name == "pointmesh_noprune" else args.reps
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--exact-child", "--samples", str(n), "--grid", str(args.grid), "--ref-chunks", str(chunks),
                                  "--reps", str(reps)], env=env, capture_output=True, text=True, check=True, timeout=600).stdout
            got = json.loads(out.strip().split("\n")[-1])
            lv = levers.setdefault(name, {"what": lab_variants.VARIANTS[name][0] if name != "product" else "the library as built",
                                          "kernels": pointmesh_kernels(env.get("TSSPLAT_AMD_LIB") or _capi.lib_path()), "runs": []})
            run = {"ref_chunks": chunks}
            for key, (q, v, f) in sides.items():
                want = rec["nearest_on_mesh"][key]
                if name == "pointmesh_count":       # tri_out holds the evaluations per query
                    run[key] = {"float64_evaluations": got[key]["tri_sum"], "share_of_pairs": got[key]["tri_sum"] / (float(n) * want["triangles"]),
                                "per_query": got[key]["tri_sum"] / float(n)}
                    assert got[key]["d2_sha256"] == want["d2_sha256"], (name, key, "not the product's d2")
                else:
                    assert (got[key]["tri_sha256"], got[key]["d2_sha256"]) == (want["tri_sha256"], want["d2_sha256"]), (name, key, "not the product's results")
                    run[key] = {"kernel_ms": got[key]["ms"], "kernel_ms_min_max": got[key]["ms_min_max"], "tri_and_d2_sha256_equal_the_products": True}
            lv["runs"].append(run)
        for name, lv in levers.items():
            if name == "pointmesh_count":
                continue
            for key in sides:
                base = statistics.median(r[key]["kernel_ms"] for r in levers["product"]["runs"])
                lv.setdefault("kernel_ms", {})[key] = statistics.median(r[key]["kernel_ms"] for r in lv["runs"])
                lv.setdefault("over_product", {})[key] = lv["kernel_ms"][key] / base
        rec["levers"] = {"order": "product, then every variant followed by the product again: fresh processes, alternating", **levers}
    # the metrics on top, beside the sampled ones
    sampled_ms, sampled_span, sampled = median_events(lambda: metrics.compare_meshes(merged.v, merged.faces, tv, tf, n=n, seed=0), args.reps)
    exact_ms, exact_span, exact = median_events(lambda: metrics.compare_meshes_exact(merged.v, merged.faces, tv, tf, n=n, seed=0), args.reps)
    rec["value"] = exact_ms
    rec["merged_against_target"] = {"compare_meshes_ms": sampled_ms, "compare_meshes_ms_min_max": sampled_span, "compare_meshes_exact_ms": exact_ms,
                                    "compare_meshes_exact_ms_min_max": exact_span, "compare_meshes_exact": "three samplings, three point-to-triangle searches, one readback",
                                    "sampled": sampled.as_dict(), "exact": exact.as_dict()}
    k = 4
    simp = simplify.simplify(merged.v, merged.faces, args.grid // k, merged.bounds)
    s_ms, _, s_rec = median_events(lambda: metrics.compare_meshes(simp.v, simp.faces, merged.v, merged.faces, n=n, seed=0), 3)
    e_ms, _, e_rec = median_events(lambda: metrics.compare_meshes_exact(simp.v, simp.faces, merged.v, merged.faces, n=n, seed=0), 3)
    rec["simplified_vs_unsimplified"] = {"factor": k, "triangles": int(simp.faces.shape[0]), "triangles_unsimplified": int(merged.faces.shape[0]), "cell": (merged.bounds[1] - merged.bounds[0]) / (args.grid // k),
                                         "compare_meshes_ms": s_ms, "compare_meshes_exact_ms": e_ms, "sampled": s_rec.as_dict(), "exact": e_rec.as_dict()}
    os.makedirs(os.path.dirname(os.path.abspath(args.exact_out)), exist_ok=True)
    runs = json.load(open(args.exact_out)) if os.path.exists(args.exact_out) else []
    runs.append(rec)
    with open(args.exact_out, "w") as fh:
        json.dump(runs, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"metric": rec["metric"], "value": rec["value"], "unit": "ms",
                      "nearest_on_mesh": {k2: {x: v2[x] for x in ("kernel_ms", "torch_over_kernel")} for k2, v2 in rec["nearest_on_mesh"].items()},
                      "compare_meshes_ms": sampled_ms, "compare_meshes_exact_ms": exact_ms}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10_000, 100_000, 200_000])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--baseline-reps", type=int, default=3)
    ap.add_argument("--samples", type=int, default=100_000, help="samples per surface of the compare_meshes run")
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_bench.json"))
    ap.add_argument("--variants", nargs="*", default=[], help="laboratory builds (tools/lab_variants.py) to price against the product at N = M = 100 000")
    ap.add_argument("--nearest-only", action="store_true", help="(the child of --variants) only the nearest part, one JSON line, no record")
    ap.add_argument("--ref-chunks", type=int, default=0, help="(the child of --variants) the chunk count of every nearest call; 0: automatic")
    ap.add_argument("--exact", action="store_true", help="time the point-to-triangle search and compare_meshes_exact instead; append to --exact-out")
    ap.add_argument("--exact-out", default=os.path.join(ROOT, "profiles", "metrics_exact_bench.json"))
    ap.add_argument("--exact-variants", nargs="*", default=[], help="laboratory builds pointmesh_* (tools/lab_variants.py) to price against the product")
    ap.add_argument("--baseline-queries", type=int, default=2048, help="--exact: queries of the torch float64 baseline where all of them would take minutes")
    ap.add_argument("--exact-child", action="store_true", help="(the child of --exact-variants) only the two searches, one JSON line, no record")
    args = ap.parse_args()
    if args.exact or args.exact_child:
        import torch
        assert torch.cuda.is_available(), "bench_metrics.py needs a GPU"
        return exact_bench(args)

    import numpy as np
    import torch
    import train_object
    import tssplat_amd.dr as dr
    from tssplat_amd import _capi, geometry, merge, metrics, scenes, spheres_init

    assert torch.cuda.is_available(), "bench_metrics.py needs a GPU"
    info = metrics.nearest_info(1, 1)
    per_lane = int(os.environ.get("BENCH_METRICS_QUERIES_PER_LANE", 0)) or info.queries_per_lane      # (a variant's, handed down by --variants)
    isa = hot_loop(os.environ.get("TSSPLAT_AMD_LIB") or _capi.lib_path(), per_lane)
    rec = {"metric": "nearest points, plain-torch chunked broadcast over the HIP kernel (N = M = the largest size)", "unit": "x", "higher_is_better": True,
           "config": {"timing": f"HIP events around each call after one warm-up; medians of {args.reps} (kernel, sampler, compare) and {args.baseline_reps} (torch) calls",
                      "points": "standard normal, float32, seeded", "block": info.block, "queries_per_lane": info.queries_per_lane, "ref_tile": info.ref_tile,
                      "peak_lane_ops_per_s": PEAK_LANE_OPS},
           "hot_loop_isa": isa, "nearest": {}}
    for n in args.sizes:
        g = torch.Generator(device="cuda").manual_seed(n)
        q, r = (torch.randn((n, 3), generator=g, device="cuda") for _ in range(2))
        ms, span, (d2, idx) = median_events(lambda: metrics.nearest(q, r, ref_chunks=args.ref_chunks), args.reps)
        base_ms, base_span, (bd2, bidx) = median_events(lambda: torch_nearest(q, r), args.baseline_reps)
        assert torch.equal(idx, bidx), f"N = M = {n}: the kernel and the torch baseline disagree on {int((idx != bidx).sum())} indices"
        assert torch.equal(d2, bd2), f"N = M = {n}: the kernel and the torch baseline disagree on d2"
        pairs = float(n) * n
        per_pair = isa["valu_per_pair"]
        rec["nearest"][str(n)] = {"kernel_ms": ms, "kernel_ms_min_max": span, "torch_ms": base_ms, "torch_ms_min_max": base_span, "torch_over_kernel": base_ms / ms,
                                  "ref_chunks": args.ref_chunks or metrics.nearest_info(n, n).auto_chunks, "pairs_per_s": pairs / (ms * 1e-3),
                                  "valu_lane_ops_per_s": per_pair * pairs / (ms * 1e-3),
                                  "fraction_of_fp32_vector_issue_rate": per_pair * pairs / (ms * 1e-3) / PEAK_LANE_OPS,
                                  "fraction_of_39.3e12_lane_ops_per_s": per_pair * pairs / (ms * 1e-3) / (PEAK_LANE_OPS / 2), "idx_identical": True}
        del q, r, d2, idx, bd2, bidx
    rec["value"] = rec["nearest"][str(args.sizes[-1])]["torch_over_kernel"]
    if args.nearest_only:
        print(json.dumps({"nearest": rec["nearest"], "hot_loop_isa": isa}))
        return
    if args.variants:
        import lab_variants
        n, levers = 100_000, {}
        for name in ["product"] + [x for v in args.variants for x in (v, "product")]:
            per_lane = int(name[len("nearest_q"):]) if name.startswith("nearest_q") else info.queries_per_lane
            chunks = -(-1024 // -(-n // (info.block * per_lane)))
            env = dict(os.environ, BENCH_METRICS_QUERIES_PER_LANE=str(per_lane))
            if name != "product":
                env["TSSPLAT_AMD_LIB"] = os.path.join(ROOT, "tssplat_amd", f"libtssplat_amd_{name}.so")
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--nearest-only", "--sizes", str(n), "--ref-chunks", str(chunks), "--reps", str(args.reps),
                                  "--baseline-reps", "1"], env=env, capture_output=True, text=True, check=True, timeout=300).stdout
            got = json.loads(out.strip().split("\n")[-1])
            levers.setdefault(name, {"what": lab_variants.VARIANTS[name][0] if name != "product" else "the library as built", "runs": []})["runs"].append(
                {"kernel_ms": got["nearest"][str(n)]["kernel_ms"], "kernel_ms_min_max": got["nearest"][str(n)]["kernel_ms_min_max"], "ref_chunks": chunks,
                 "vgpr_count": got["hot_loop_isa"]["vgpr_count"], "scratch_bytes": got["hot_loop_isa"]["scratch_bytes"], "lds_bytes": got["hot_loop_isa"]["lds_bytes"],
                 "valu_per_pair": got["hot_loop_isa"]["valu_per_pair"], "idx_identical_to_torch": True})
        base = statistics.median(r["kernel_ms"] for r in levers["product"]["runs"])
        for name, lv in levers.items():
            lv["kernel_ms"] = statistics.median(r["kernel_ms"] for r in lv["runs"])
            lv["over_product"] = lv["kernel_ms"] / base
        rec["levers"] = {"n": n, "m": n, "order": "product, then every variant followed by the product again: fresh processes, alternating", **levers}

    # the merged mario scene against its target
    tgt = np.load(os.path.join(ROOT, "tests", "golden", "mario_mesh.npz"))
    tv = torch.from_numpy(tgt["vertices"].astype(np.float32)).cuda()
    tf = torch.from_numpy(tgt["faces"].astype(np.int32)).cuda()
    mvp = torch.from_numpy(scenes.dataset_mvps(120)).cuda()
    with torch.no_grad():
        target = train_object.render_alpha(dr.RasterizeCudaContext(), tv, tf, mvp, 512).clone()
    kp = spheres_init.init_spheres(target, mvp, 20, grid=72)
    geo = geometry.TetMeshMultiSphereGeometry(kp, k=8)
    merged = merge.merge_tets(geo.tet_v.detach().contiguous(), geo.tet_elem, grid=args.grid)
    n = args.samples
    sample_ms, sample_span, sa = median_events(lambda: metrics.sample_surface(merged.v, merged.faces, n, 0), args.reps)
    sb = metrics.sample_surface(tv, tf, n, 0)
    compare_ms, compare_span, _ = median_events(lambda: metrics.compare(sa, sb), args.reps)
    meshes_ms, meshes_span, got = median_events(lambda: metrics.compare_meshes(merged.v, merged.faces, tv, tf, n=n, seed=0), args.reps)
    raw = geo.surface_metrics(tv, tf, n=n, seed=0)
    rec["merged_mario"] = {"workload": f"mario fixture, {len(kp)} initial tet-spheres x kuhn8 merged at grid {args.grid}: {int(merged.faces.shape[0])} triangles, against "
                                       f"the target mesh ({int(tf.shape[0])} triangles); {n} samples per surface",
                           "sample_surface_ms": sample_ms, "sample_surface_ms_min_max": sample_span, "compare_ms": compare_ms, "compare_ms_min_max": compare_span,
                           "compare_meshes_ms": meshes_ms, "compare_meshes_ms_min_max": meshes_span,
                           "compare_meshes": "three samplings, four nearest calls, two readbacks of a record", "merged": got.as_dict(),
                           "raw_union_of_the_initial_spheres": raw.as_dict()}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"metric": rec["metric"], "value": rec["value"], "unit": "x", "nearest": rec["nearest"], "hot_loop_isa": isa,
                      "merged_mario": {k: v for k, v in rec["merged_mario"].items() if k.endswith("_ms")}}))


if __name__ == "__main__":
    main()
