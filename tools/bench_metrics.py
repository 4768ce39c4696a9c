#!/usr/bin/env python3
"""The surface metrics, timed: `metrics.sample_surface`, `metrics.nearest` and `metrics.compare`, and one `compare_meshes` of the
grid-256 merged mario scene against its target mesh.

    python tools/bench_metrics.py [--sizes 10000 100000 200000 --reps 7 --baseline-reps 3 --out profiles/metrics_bench.json]
                                  [--variants nearest_q2 nearest_q8 nearest_tile256 nearest_tile4096 nearest_minscan]

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
    args = ap.parse_args()

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
