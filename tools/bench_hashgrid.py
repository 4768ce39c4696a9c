#!/usr/bin/env python3
"""The texture stage's hash-grid encoding on one GPU: the HIP kernels (tssplat_amd.encoding) against a plain-torch restatement of
the same semantics (gathers + index_add_, kept here and not in the product), forward and forward + backward (dL/dparams).

Workloads, both with the default ExplicitMaterial config (16 levels, F = 2, T = 2^19, base 16):
  texture  the foreground pixels, in pixel order, of tests/golden/mario_mesh.npz under scenes.dataset_mvps(views) at res^2,
           mapped into [0, 1]^3 as contract_to_unisphere does;
  random   as many uniform random points in [0, 1]^3 (the worst case: no two neighbouring lanes share a cell).

    python tools/bench_hashgrid.py [--views 120 --res 512 --reps 10] [--param-grad atomic|sorted|planned|both] [--no-torch]

--param-grad picks the route to dL/dparams that the HIP numbers are taken with (default: atomic; ``planned``: one point plan
built before the timing, every backward through it).  ``both`` times all three routes on the same inputs in one run (HIP-event
medians over --reps), reports sorted / atomic and planned / sorted / atomic, the sorted route's workspace and its per-kernel
split (key pass, each radix pass = histogram + scan + scatter, segmented sum + fold; torch.profiler kernel times), and for the
planned route the plan-build time, the plan's bytes, its per-kernel split and the bytes per second of its sum kernel.
--no-torch skips the plain-torch restatement (minutes at the texture workload) and the fields that compare against it.

One JSON line per workload: Mpoints/s, ms, the gather and atomic-add bytes per second, the speed-up, the torch path's per-level
split and the largest difference between the two paths.  Byte counts are nominal (8 corners x F x 4 B per point and level)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16,
           "per_level_scale": 1.447269237440378}
PRIMES = (1, 2654435761, 805459861)


def texture_points(views: int, res: int) -> torch.Tensor:
    from tssplat_amd import dr, scenes
    m = np.load(os.path.join(ROOT, "tests", "golden", "mario_mesh.npz"))
    v = torch.from_numpy(m["vertices"].astype(np.float32)).cuda()
    tri = torch.from_numpy(m["faces"].astype(np.int32)).cuda()
    mvp = torch.from_numpy(scenes.dataset_mvps(views).astype(np.float32)).cuda()
    pos = torch.matmul(torch.cat([v, torch.ones_like(v[:, :1])], 1), mvp.transpose(1, 2)).contiguous()
    rast, _ = dr.rasterize(dr.RasterizeCudaContext(), pos, tri, resolution=[res, res], grad_db=False)
    p, _ = dr.interpolate(v[None], rast, tri)
    return ((p[rast[..., 3] > 0] + 1) * 0.5).contiguous()


class TorchGrid:
    """The encoding restated with torch ops: per level, 8 corner indices (int64 arithmetic masked to uint32), gathers, weights;
    backward = index_add_ of weight x dL/dy into the table."""

    def __init__(self, layout, F):
        self.lay, self.F = layout, F

    def corners(self, x, l):
        M = 0xFFFFFFFF
        scale = float(self.lay["scale"][l])
        pos = torch.addcmul(torch.full_like(x, 0.5), x, torch.full_like(x, scale))
        fl = torch.floor(pos)
        cell = fl.to(torch.int64) & M
        frac = pos - fl
        res, entries, hashed = int(self.lay["res"][l]), int(self.lay["offset"][l + 1] - self.lay["offset"][l]), bool(self.lay["is_hash"][l])
        out = []
        for c in range(8):
            b = [(c >> d) & 1 for d in range(3)]
            cx, cy, cz = [(cell[:, d] + b[d]) & M for d in range(3)]
            if hashed:
                i = (cx * PRIMES[0] & M) ^ (cy * PRIMES[1] & M) ^ (cz * PRIMES[2] & M)
            else:
                i = (cx + cy * res + (cz * ((res * res) & M) & M)) & M
            w = torch.ones_like(frac[:, 0])
            for d in range(3):
                w = w * (frac[:, d] if b[d] else 1.0 - frac[:, d])
            out.append((i % entries + int(self.lay["offset"][l]), w))
        return out

    def forward(self, x, P, levels=None):
        Pv = P.view(-1, self.F)
        cols, saved = [], []
        for l in (range(len(self.lay["res"])) if levels is None else levels):
            acc = torch.zeros(x.shape[0], self.F, device=x.device)
            cs = self.corners(x, l)
            for i, w in cs:
                acc += w[:, None] * Pv.index_select(0, i)
            cols.append(acc)
            saved.append((l, cs))
        return torch.cat(cols, 1), saved

    def backward(self, saved, g, n_params):
        gP = torch.zeros(n_params // self.F, self.F, device=g.device)
        for k, (l, cs) in enumerate(saved):
            gl = g[:, k * self.F:(k + 1) * self.F]
            for i, w in cs:
                gP.index_add_(0, i, w[:, None] * gl)
        return gP.view(-1)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def timed_median(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def sorted_kernel_split(fn):
    """Device time of one call of ``fn`` per stage of the sorted route, from torch.profiler's kernel records in launch order:
    a key kernel opens a level, every scatter closes a radix pass."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    evs = sorted((e for e in prof.events() if "grid_sorted_" in e.name), key=lambda e: e.time_range.start)
    split, p = {}, 0
    for e in evs:
        us = e.device_time if hasattr(e, "device_time") else e.cuda_time
        if "key_kernel" in e.name:
            stage, p = "key_pass", 0
        elif "sum_kernel" in e.name or "fold_kernel" in e.name:
            stage = "segmented_sum"
        else:
            stage = f"radix_pass_{p}"
            p += "scatter_kernel" in e.name
        split[stage] = split.get(stage, 0.0) + us / 1e3
    return {k: round(v, 3) for k, v in sorted(split.items())}, len(evs)


def planned_kernel_split(fn):
    """Device time of one call of ``fn`` per kernel of the planned route (torch.profiler), and the number of launches."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    evs = [e for e in prof.events() if "grid_planned_" in e.name]
    split = {}
    for e in evs:
        us = e.device_time if hasattr(e, "device_time") else e.cuda_time
        stage = "segmented_sum" if "sum_kernel" in e.name else ("fold" if "fold_kernel" in e.name else e.name.split("(")[0])
        split[stage] = split.get(stage, 0.0) + us / 1e3
    return {k: round(v, 3) for k, v in sorted(split.items())}, len(evs)


def bench(name, x, reps, param_grad="atomic", with_torch=True):
    from tssplat_amd import encoding
    enc = encoding.GridEncoding(3, DEFAULT, param_grad="sorted" if param_grad == "sorted" else "atomic").cuda()
    with torch.no_grad():
        enc.params.uniform_(-1, 1)
    lay = enc.layout
    F, L = 2, 16
    N = int(x.shape[0])
    g = torch.randn(N, L * F, device="cuda")
    tg = TorchGrid(lay, F)

    def hip_fwd():
        with torch.no_grad():
            return enc(x)

    plan = enc.plan_points(x) if param_grad == "planned" else None

    def hip_fb():
        enc.params.grad = None
        enc(x if plan is None else plan).backward(g)

    def torch_fwd():
        with torch.no_grad():
            return tg.forward(x, enc.params)[0]

    def torch_fb():
        with torch.no_grad():
            y, saved = tg.forward(x, enc.params)
            return tg.backward(saved, g, lay["n_params"])

    t_hf, t_hfb = timed(hip_fwd, reps), timed(hip_fb, reps)
    gather = N * L * 8 * F * 4
    rec = {
        "workload": name, "points": N, "reps": reps, "param_grad": "planned" if plan is not None else enc.cfg["param_grad"],
        "hip_fwd_ms": round(t_hf, 3), "hip_fwd_bwd_ms": round(t_hfb, 3), "hip_bwd_ms": round(t_hfb - t_hf, 3),
        "hip_fwd_mpoints_per_s": round(N / t_hf / 1e3, 1), "hip_fwd_bwd_mpoints_per_s": round(N / t_hfb / 1e3, 1),
        "hip_fwd_gather_tb_per_s": round(gather / t_hf / 1e9, 3),
        "hip_bwd_nominal_atomic_tb_per_s": round(gather / max(t_hfb - t_hf, 1e-6) / 1e9, 3),
        "guide_ceilings_tb_per_s": {"atomic_add_f32_256B_rows": 1.3, "atomic_add_f32_64_rows_per_wave": 0.08, "random_row_gather_mall": 8.6},
    }
    gp_t = None
    if with_torch:
        t_tf, t_tfb = timed(torch_fwd, max(1, reps // 5)), timed(torch_fb, max(1, reps // 5))
        levels = {}
        for l in range(L):
            levels[l] = round(timed(lambda: tg.forward(x, enc.params, levels=[l]), 1), 3)
        y_h, y_t = hip_fwd(), torch_fwd()
        hip_fb()
        gp_t = torch_fb()
        rec.update({
            "torch_fwd_ms": round(t_tf, 3), "torch_fwd_bwd_ms": round(t_tfb, 3),
            "speedup_fwd": round(t_tf / t_hf, 2), "speedup_fwd_bwd": round(t_tfb / t_hfb, 2),
            "torch_fwd_ms_per_level": levels,
            "max_abs_diff_fwd": float((y_h - y_t).abs().max()),
            "max_abs_diff_dparams": float((enc.params.grad - gp_t).abs().max()),
            "max_abs_dparams": float(gp_t.abs().max()),
        })
    if param_grad == "both":
        other = encoding.GridEncoding(3, DEFAULT, param_grad="sorted").cuda()
        with torch.no_grad():
            other.params.copy_(enc.params)

        def sorted_fb():
            other.params.grad = None
            other(x).backward(g)

        t_fwd = timed_median(hip_fwd, reps)
        t_atomic, t_sorted = timed_median(hip_fb, reps), timed_median(sorted_fb, reps)
        sorted_fb()
        first = other.params.grad.clone()
        sorted_fb()
        try:
            split, n_kernels = sorted_kernel_split(sorted_fb)
        except Exception as e:                                        # (a profiler that is not there is said, not hidden)
            split, n_kernels = f"torch.profiler failed: {e!r}", 0
        records = N * L * 8
        rec["param_grad_compare"] = {
            "fwd_ms_median": round(t_fwd, 3),
            "atomic_fwd_bwd_ms_median": round(t_atomic, 3), "sorted_fwd_bwd_ms_median": round(t_sorted, 3),
            "atomic_bwd_ms": round(t_atomic - t_fwd, 3), "sorted_bwd_ms": round(t_sorted - t_fwd, 3),
            "sorted_over_atomic_fwd_bwd": round(t_sorted / t_atomic, 3),
            "sorted_over_atomic_bwd": round((t_sorted - t_fwd) / max(t_atomic - t_fwd, 1e-6), 3),
            "sorted_workspace_bytes": encoding.sorted_workspace_bytes(other.cfg, N),
            "sorted_records": records, "sorted_kernel_ms": split, "sorted_kernel_launches": n_kernels,
            "sorted_repeats_bitwise": bool(torch.equal(first, other.params.grad)),
        }
        if gp_t is not None:
            rec["param_grad_compare"]["sorted_max_abs_diff_dparams"] = float((other.params.grad - gp_t).abs().max())

        # the planned route on the same inputs: one plan, built (and timed) here, then every backward through it
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        build_ms = []
        for _ in range(3):
            a.record()
            pplan = other.plan_points(x)
            b.record()
            torch.cuda.synchronize()
            build_ms.append(a.elapsed_time(b))

        def planned_fb():
            other.params.grad = None
            other(pplan).backward(g)

        t_planned = timed_median(planned_fb, reps)
        planned_fb()
        try:
            psplit, pn = planned_kernel_split(planned_fb)
        except Exception as e:
            psplit, pn = f"torch.profiler failed: {e!r}", 0
        bwd_a, bwd_s, bwd_p = t_atomic - t_fwd, t_sorted - t_fwd, t_planned - t_fwd
        # what the sum kernel moves, nominally: 4 B of plan, 12 B of x and F * 4 B of g per record
        sum_bytes = records * (4 + 12 + F * 4)
        sum_ms = psplit.get("segmented_sum") if isinstance(psplit, dict) else None
        rec["param_grad_compare"].update({
            "planned_fwd_bwd_ms_median": round(t_planned, 3), "planned_bwd_ms": round(bwd_p, 3),
            "planned_over_sorted_bwd": round(bwd_p / max(bwd_s, 1e-6), 3), "planned_over_atomic_bwd": round(bwd_p / max(bwd_a, 1e-6), 3),
            "plan_build_ms": round(float(np.median(build_ms)), 3), "plan_bytes": pplan.nbytes,
            "plan_repaid_after_iterations_vs_sorted": (round(float(np.median(build_ms)) / (bwd_s - bwd_p), 2) if bwd_s > bwd_p else None),
            "plan_repaid_after_iterations_vs_atomic": (round(float(np.median(build_ms)) / (bwd_a - bwd_p), 2) if bwd_a > bwd_p else None),
            "planned_workspace_bytes": encoding.planned_workspace_bytes(other.cfg, N),
            "planned_kernel_ms": psplit, "planned_kernel_launches": pn,
            "planned_sum_nominal_tb_per_s": (round(sum_bytes / sum_ms / 1e9, 3) if sum_ms else None),
            "guide_plain_streaming_tb_per_s": 6.0,
            "planned_equals_sorted_bitwise": bool(torch.equal(first, other.params.grad)),
        })
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=120)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--param-grad", choices=("atomic", "sorted", "planned", "both"), default="atomic")
    ap.add_argument("--no-torch", action="store_true", help="skip the plain-torch restatement and the comparisons against it")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    pts = texture_points(a.views, a.res)
    recs = [bench(f"texture_{a.views}x{a.res}", pts, a.reps, a.param_grad, not a.no_torch)]
    g = torch.Generator(device="cuda").manual_seed(0)
    recs.append(bench("random_unit_cube", torch.rand(pts.shape[0], 3, device="cuda", generator=g), a.reps, a.param_grad, not a.no_torch))
    for r in recs:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(recs, fh, indent=1)


if __name__ == "__main__":
    main()
