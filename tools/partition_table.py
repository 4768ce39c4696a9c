"""Host-only plan table of the three large scenes (no GPU): what the partitioner makes of 512 x kuhn19, 952 x a.veg and
540 x delaunay6000, and how long the constructor takes.

    python tools/partition_table.py --column cells_fm --out profiles/r08_partition_plan.json

writes (or updates) one column of the JSON file: ``plan_info()`` of ``TetSpheres(..., host_only=True, num_threads=8)`` per scene
plus ``plan_s``, the constructor's wall time on this host.  Run it once per build (select another library with
TSSPLAT_AMD_LIB) and give every build its own column name."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SCENES = {"kuhn19x512": ("kuhn19", 512), "avegx952": ("aveg", 952), "delaunay6000x540": ("delaunay6000", 540)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--column", required=True, help="name of the column (the build) the figures are filed under")
    ap.add_argument("--out", required=True)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--scenes", nargs="*", default=list(SCENES))
    args = ap.parse_args()
    from tssplat_amd import scenes, tet_spheres_ext as ext
    doc = {"scenes": {}}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            doc = json.load(fh)
    for name in args.scenes:
        kind, n = SCENES[name]
        sc = scenes.make_scene(kind, n)
        rest, tets = sc.rest.reshape(-1), sc.tets.reshape(-1)
        t0 = time.perf_counter()
        ts = ext.TetSpheres(rest, tets, host_only=True, num_threads=args.threads)
        plan_s = time.perf_counter() - t0
        info = ts.plan_info()
        info.pop("device_bytes", None)
        info["slots_per_tet"] = info["total_slots"] / info["n_tets"]
        info["plan_s"] = round(plan_s, 3)
        # what the gate of the partition work compares: slots + 0.28 x staged rows (3.9 ps per row over 13.7 ps per slot)
        info["slots_plus_028_rows"] = round(info["total_slots"] + 0.28 * info["shared_vertex_copies"], 1)
        doc["scenes"].setdefault(name, {})[args.column] = info
        print(name, args.column, json.dumps(info), flush=True)
        ts.close()
    doc["what"] = (f"host-only plans (TetSpheres(..., host_only=True, num_threads={args.threads}).plan_info()), one column per build; "
                   "plan_s = wall time of the constructor on this host")
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
