#!/usr/bin/env python3
"""The fused MLP (tssplat_amd.network, csrc/mlp_kernels.hip) on one GPU against this repo's VanillaMLP (fp32 nn.Linear, the
texture stage's default) and a torch fp16 nn.Linear chain of the same shape, forward and forward + backward (dL/dparams and
dL/dx).

Configs: 32 -> 64 -> 3 (L = 1, the texture stage's), 32 -> 64 -> 64 -> 3 (L = 2) and 3 -> 128 x 5 -> 3 (tiny-cuda-nn's
default); rows: 131 072, 1 M and 3.92 M (the mario foreground at 120 x 512^2).

    python tools/bench_mlp.py [--reps 20] [--rows 131072,1048576,3920000]

One JSON line per (config, rows): median ms of each path (HIP events around each call), the speed-ups over fp32 torch, and
the fused path's algorithmic bytes (read x, write y; backward: read x and dy, write dx) per second."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [(32, 3, 64, 1), (32, 3, 64, 2), (3, 3, 128, 5)]


def timed(fn, reps):
    """Median over `reps` of HIP-event times around one call (after two warm-up calls)."""
    fn()
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def run(n_in, n_out, W, L, N, reps):
    from tssplat_amd import models, tcnn
    cfg = {"otype": "FullyFusedMLP", "n_neurons": W, "n_hidden_layers": L, "activation": "ReLU", "output_activation": "None"}
    fused = tcnn.Network(n_in, n_out, cfg).cuda()
    vanilla = models.VanillaMLP(n_in, n_out, {"n_neurons": W, "n_hidden_layers": L}).cuda()
    half = models.VanillaMLP(n_in, n_out, {"n_neurons": W, "n_hidden_layers": L}).cuda().half()
    x = torch.rand(N, n_in, device="cuda") * 2 - 1
    xh = x.half()
    dy = torch.randn(N, n_out, device="cuda")
    dyh = dy.half()

    def fb(net, inp, g):
        def f():
            xi = inp.detach().requires_grad_(True)
            net(xi).backward(g)
        return f

    def fwd(net, inp):
        def f():
            with torch.no_grad():
                net(inp)
        return f
    res = {"config": f"{n_in}->{W}x{L}->{n_out}", "rows": N}
    ms = {"fused_fwd": timed(fwd(fused, x), reps), "fp32_torch_fwd": timed(fwd(vanilla, x), reps),
          "fp16_torch_fwd": timed(fwd(half.layers, xh), reps),
          "fused_fwd_bwd": timed(fb(fused, x, dy), reps), "fp32_torch_fwd_bwd": timed(fb(vanilla, x, dy), reps),
          "fp16_torch_fwd_bwd": timed(fb(half.layers, xh, dyh), reps)}
    res["median_ms"] = {k: round(v, 4) for k, v in ms.items()}
    res["speedup_vs_fp32_torch"] = {"fwd": round(ms["fp32_torch_fwd"] / ms["fused_fwd"], 2),
                                    "fwd_bwd": round(ms["fp32_torch_fwd_bwd"] / ms["fused_fwd_bwd"], 2)}
    fb_bytes = 4 * N * (n_in + n_out)
    res["fused_algorithmic_GBps"] = {"fwd": round(fb_bytes / ms["fused_fwd"] / 1e6, 1),
                                     "fwd_bwd": round((fb_bytes + 4 * N * (n_in + n_out) + 4 * N * n_in) / ms["fused_fwd_bwd"] / 1e6, 1)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", default="131072,1048576,3920000")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    for n_in, n_out, W, L in CONFIGS:
        for N in [int(v) for v in a.rows.split(",")]:
            print(json.dumps(run(n_in, n_out, W, L, N, a.reps)), flush=True)


if __name__ == "__main__":
    main()
