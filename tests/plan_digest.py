"""SHA-256 digests over everything the C ABI shows of a tiling plan -- a TEST helper shared by tests/test_plan_bytes.py and
tests/golden/make_golden.py (which records tests/golden/plan_digests.json).

The planner is pure host code and a plan is plain data, so a refactor of the planner must leave these digests as they are.
Every case also hashes its inputs: a different numpy (another random stream, another scene generator) then shows up as an
input difference, not as a planner change."""
from __future__ import annotations

import hashlib
import os

import numpy as np

import tile_emulator as TE

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_digests.json")

# (scene, spheres, options, operator): the committed cases -- lattices, the cone and a.veg only (Delaunay scenes depend on the
# installed Qhull).  operator: None, "symmetric" or "nonsymmetric", the constructions of tests/test_operator.py.
CASES = [
    ("kuhn8", 3, {}, None),
    ("kuhn8", 2, dict(lds_budget_bytes=40000), None),
    ("kuhn3", 40, {}, None),
    ("kuhn12", 3, {}, None),
    ("kuhn12", 1, dict(max_threads=256, lds_budget_bytes=40960), None),
    ("kuhn12", 1, dict(debug_flags=2), None),
    ("kuhn12", 2, dict(debug_flags=4), None),
    ("kuhn12", 1, dict(lane_search_sweeps=-1), None),
    ("kuhn12", 2, dict(rebuild_dminv=True), None),
    ("kuhn12", 1, dict(slots_per_thread=3, max_threads=512), None),
    ("kuhn8", 2, dict(slots_per_thread=4, max_threads=768, lds_budget_bytes=163840), None),
    ("cone", 2, {}, None),
    ("cone", 1, dict(lds_budget_bytes=30000), None),
    ("kuhn19", 3, {}, None),
    ("kuhn19", 2, dict(num_threads=1), None),
    ("aveg", 2, {}, None),
    ("kuhn8", 2, {}, "symmetric"),
    ("kuhn8", 2, {}, "nonsymmetric"),
]

# run by hand on both trees of a planner change (make_golden.py plan_digests --extra), not committed
EXTRA_CASES = [
    ("delaunay2500", 3, {}, None),
    ("delaunay2500", 1, dict(lds_budget_bytes=50000, max_threads=512), None),
    ("kuhn19", 64, {}, None),
]


def case_id(kind, spheres, kw, operator):
    opts = ",".join(f"{k}={int(v) if isinstance(v, bool) else v}" for k, v in sorted(kw.items()))
    return f"{kind}x{spheres}" + (f"[{opts}]" if opts else "") + (f"+{operator}" if operator else "")


def make_inputs(kind, spheres, operator):
    """(rest float32 [n,3], tets int32 [m,4], scipy CSR operator or None)"""
    from oracle import tet_energy_oracle as O
    from tssplat_amd import scenes
    if kind == "aveg":          # replicated as in tests/test_plan_host.py::test_real_mesh_plan
        z = np.load(os.path.join(os.path.dirname(GOLDEN), "aveg_mesh.npz"))
        sc = scenes.replicate_spheres(z["rest"].astype(np.float64), z["tets"], spheres, seed=3)
    else:
        sc = scenes.make_scene(kind, spheres)
    rest = np.ascontiguousarray(sc.rest, dtype=np.float32)
    tets = np.ascontiguousarray(sc.tets, dtype=np.int32)
    L = None
    if operator is not None:
        import test_operator
        nbr = O.face_adjacency(sc.tets)
        L = test_operator.random_operator(nbr, np.random.default_rng(5), symmetric=True) if operator == "symmetric" \
            else O.element_laplacian_scaled(nbr).tocsr()
    return rest, tets, L


def input_digest(rest, tets, L):
    h = hashlib.sha256()
    h.update(rest.tobytes())
    h.update(tets.tobytes())
    if L is not None:
        for a, dt in ((L.indptr, np.int64), (L.indices, np.int32), (L.data, np.float64)):
            h.update(np.ascontiguousarray(a, dtype=dt).tobytes())
    return h.hexdigest()


def plan_digest(ts):
    """Everything the ABI exposes: plan_info(), every tile's scalar fields and arrays, the finish lists, the adjacency and
    index_reps()."""
    h = hashlib.sha256()

    def put(name, a):
        a = np.ascontiguousarray(a)
        h.update(f"{name}:{a.dtype.str}:{a.shape};".encode())
        h.update(a.tobytes())

    h.update(repr(sorted(ts.plan_info().items())).encode())
    for T in TE.plan_tiles(ts):
        h.update(repr([(k, int(T[k])) for k in ("n_slots", "n_owned", "s_pad", "n_verts", "n_excl", "stage_off", "n_rows", "rec_base")]).encode())
        for k in ("planes", "row_start", "gvid", "vdst", "slot_tet"):
            put(k, T[k])
        put("rest", T["rest"] if T["rest"] is not None else np.zeros(0, np.float32))
    for name, a in zip(("fin_vid", "fin_off", "fin_idx"), TE.finish_lists(ts)):
        put(name, a)
    put("adjacency", TE.adjacency(ts))
    put("index_reps", ts.index_reps())
    return h.hexdigest()


def digests(kind, spheres, kw, operator):
    from tssplat_amd import tet_spheres_ext as ext
    rest, tets, L = make_inputs(kind, spheres, operator)
    ts = ext.TetSpheres(rest.reshape(-1), tets.reshape(-1), host_only=True, operator=L, **kw)
    return {"inputs": input_digest(rest, tets, L), "plan": plan_digest(ts)}
