#!/usr/bin/env python3
"""Host-side estimate of the tile kernel's LDS bank-conflict cycles, from the plan alone (no GPU).

Replays the addresses of the data-dependent LDS accesses (neighbour gathers of passes 2/3, position reads of pass 1, the
scatter of the corner forces into the per-vertex force array) through the lane-group / bank rules of MI355X_MICROARCH.md (LDS
section) and reports base cycles and extra (conflict) cycles per tile slot.  Used to compare ordering heuristics in
csrc/plan_planes.cpp offline (round 5: the scatter's ranks, 2.8x -> 1.5x the conflict-free cycles).  The per-vertex sums read
consecutive entries per lane and are conflict-free by construction.

    python tools/lds_conflicts.py [--scene kuhn19 --spheres 1] [--no-conflict-aware]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

G128 = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
        [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
G128 = G128 + [[l + 32 for l in g] for g in G128]


def group_cycles(keys, addrs):
    """LDS cycles of one lane group: max over banks of the number of distinct addresses on that bank."""
    if len(keys) == 0:
        return 0
    pairs = np.unique(np.stack([keys, addrs], axis=1), axis=0)
    return int(np.bincount(pairs[:, 0]).max())


def tile_conflicts(T, spt, nthr=768):
    sp = T["s_pad"]
    nq = sp // spt
    pl = T["planes"]
    slots_all = np.arange(sp)
    item = (slots_all % spt) * nq + slots_all // spt            # = LDS record index; the items below n_owned are the owned ones
    owned_slot = item < T["n_owned"]
    real = T["slot_tet"] >= 0
    rb = T["rec_base"]
    nb = (np.stack([pl[2] & 0xffff, pl[2] >> 16, pl[3] & 0xffff, pl[3] >> 16], axis=1).astype(np.int64) - rb // 4) // 12
    f16 = np.stack([pl[0] & 0xffff, pl[0] >> 16, pl[1] & 0xffff, pl[1] >> 16], axis=1).astype(np.int64)
    lv, rank = f16 & 0x3ff, f16 >> 10
    ent = T["row_start"].astype(np.int64)[rank] + lv
    res = dict(g128_base=0, g128_extra=0, g32_base=0, g32_extra=0, pos_base=0, pos_extra=0, sc_base=0, sc_extra=0)
    col0 = (rb // 16) % 16                                       # the record region starts at a 16-byte column of its own
    for p in range(spt):
        for wbase in range(0, nq, 64):
            lanes = np.arange(wbase, min(wbase + 64, nq))
            slots = spt * lanes + p
            for owned_only in (True, False):                 # pass 2 (owned lanes), pass 3 (all lanes)
                act = owned_slot[slots] if owned_only else np.ones(len(slots), bool)
                if not act.any():
                    continue
                for k in range(4):
                    idx = nb[slots, k]
                    for g in G128:                            # the two b128 quads of the record
                        sel = [i for i in range(len(lanes)) if (lanes[i] - wbase) in g and act[i]]
                        if not sel:
                            continue
                        c = group_cycles((3 * idx[sel] + col0) % 16, idx[sel])
                        res["g128_base"] += 2
                        res["g128_extra"] += 2 * (c - 1)
                    for h in range(2):                        # the rotated tail dword
                        sel = [i for i in range(len(lanes)) if (lanes[i] - wbase) // 32 == h and act[i]]
                        if not sel:
                            continue
                        ii = idx[sel]
                        bank = (rb // 4 + 12 * ii + ((ii >> 3) & 3)) % 32
                        c = group_cycles(bank, ii)
                        res["g32_base"] += 1
                        res["g32_extra"] += c - 1
            for k in range(4):
                # pass 1: one ds_read_b128 of a staged position per corner (16-byte columns: 8 per cycle)
                for g in G128:
                    sel = [i for i in range(len(lanes)) if (lanes[i] - wbase) in g and real[slots[i]]]
                    if sel:
                        v = lv[slots[sel], k]
                        res["pos_base"] += 1                  # 16 lanes x 16 bytes over the sixteen 16-byte columns (64 banks)
                        res["pos_extra"] += group_cycles(v % 16, v) - 1
                # scatter: ds_write2_b32 (dwords 3e, 3e + 1) + ds_write_b32 (3e + 2) per corner, 32 lanes per cycle group
                for h in range(2):
                    sel = [i for i in range(len(lanes)) if (lanes[i] - wbase) // 32 == h and real[slots[i]]]
                    if not sel:
                        continue
                    e = ent[slots[sel], k]
                    b2 = int(np.bincount(np.concatenate([(3 * e) % 32, (3 * e + 1) % 32]), minlength=32).max())
                    b1 = int(np.bincount((3 * e + 2) % 32, minlength=32).max())
                    base = -(-2 * len(sel) // 32) + -(-len(sel) // 32)
                    res["sc_base"] += base
                    res["sc_extra"] += b2 + b1 - base
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="kuhn19")
    ap.add_argument("--spheres", type=int, default=1)
    ap.add_argument("--no-conflict-aware", action="store_true")
    ap.add_argument("--max-tiles", type=int, default=12)
    ap.add_argument("--lane-sweeps", type=int, default=0, help="tsamd_options.lane_search_sweeps (0 = default, -1 = none)")
    args = ap.parse_args()
    from tssplat_amd import scenes, tet_spheres_ext as X
    import tile_emulator as TE
    sc = scenes.make_scene(args.scene, args.spheres)
    ts = X.TetSpheres(sc.rest.reshape(-1), sc.tets.reshape(-1), host_only=True,
                      debug_flags=2 if args.no_conflict_aware else 0, lane_search_sweeps=args.lane_sweeps)
    spt = ts.plan_info()["slots_per_thread"]
    tot, slots = {}, 0
    for i, T in enumerate(TE.plan_tiles(ts)):
        if i >= args.max_tiles:
            break
        r = tile_conflicts(T, spt, ts.plan_info()["block_threads"])
        slots += T["n_slots"]
        for k, val in r.items():
            tot[k] = tot.get(k, 0) + val
    print(f"{args.spheres} x {args.scene}: {slots} slots in the first {min(i + 1, args.max_tiles)} tiles; LDS cycles per 64 slots:")
    for k, what in (("g128", "neighbour gathers, b128 quads"), ("g32", "neighbour gathers, tail dword"), ("pos", "position reads (pass 1)"),
                    ("sc", "scatter of the corner forces")):
        b, e = tot[k + "_base"] * 64 / slots, tot[k + "_extra"] * 64 / slots
        print(f"  {k:5s} base {b:7.1f}  conflict extra {e:7.1f}  ({(b + e) / b:.2f}x)   {what}")


if __name__ == "__main__":
    main()
