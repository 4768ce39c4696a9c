"""The exact point-to-triangle search (tssplat_amd/metrics.py: nearest_on_mesh, compare_meshes_exact; tsamd_nearest_on_mesh).  The device
results are compared with tests/pointmesh_oracle.py bit for bit on d2, tri and point.  The oracle itself is checked on the CPU against
exact rational arithmetic, in every Voronoi region and on every boundary between them, and on a mesh of hostile triangles."""
import ctypes as C
import functools
import inspect
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

import metrics_oracle as MO
import pointmesh_oracle as PO
from tssplat_amd import _build, _capi

gpu = pytest.mark.gpu
INVALID = 1     # TSAMD_ERR_INVALID_ARGUMENT
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
U32 = 2.0 ** -24            # unit roundoff of float32
U64 = 2.0 ** -53            # and of float64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------- meshes ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden(name):
    d = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    return np.ascontiguousarray(d["vertices"], dtype=F32), np.ascontiguousarray(d["faces"], dtype=np.int32)


def _hostile_mesh():
    """tests/test_metrics.py's hostile mesh.  Triangle 0: area 1/2 (w = 1).  1: zero area (repeated corner).  2: a NaN vertex.  3: an index past
    the end.  4: a negative index.  5: w = 2^-34.  6: collinear corners.  7: area 1/8 (w = 1/4).  8: an infinite vertex."""
    s = 2.0 ** -17
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [5, 5, 5], [5 + s, 5, 5], [5, 5 + s, 5], [2, 2, 2], [3, 3, 3], [4, 4, 4],
                  [0, 0, 1], [0.5, 0, 1], [0, 0.5, 1], [np.inf, 0, 0]], F32)
    f = np.array([[0, 1, 2], [0, 1, 1], [0, 3, 2], [0, 1, 14], [0, -1, 2], [4, 5, 6], [7, 8, 9], [10, 11, 12], [0, 13, 2]], np.int32)
    return v, f


HOSTILE_VALID = (0, 5, 7)


def _hostile_queries():
    q = np.array([[0.25, 0.25, 0.1], [5, 5, 5.5], [0.1, 0.1, 0.9], [3, 3, 3], [5 + 2.0 ** -18, 5 + 2.0 ** -19, 4], [-7, 2, 0.5], [0, 0, 0.5],
                  [np.nan, 0, 0], [0, np.nan, 0], [1, 2, np.nan], [np.inf, 0, 0], [0, -np.inf, 1], [3e38, 3e38, -3e38], [1e18, 0, 0]], F32)
    return q


def _lattice_mesh(T):
    """T isolated right triangles with unit legs on the integer lattice of the plane z = 0: equal areas, every coordinate exact."""
    t = np.arange(T)
    v = np.zeros((T, 3, 3), F32)
    v[:, :, 0] = (2 * (t % 16))[:, None]
    v[:, :, 1] = (2 * (t // 16))[:, None]
    v[:, 1, 0] += 1
    v[:, 2, 1] += 1
    return v.reshape(-1, 3), np.arange(3 * T, dtype=np.int32).reshape(T, 3)


def _lattice_queries(n, T, seed):
    """Points on a grid of 1/8 steps over the lattice of T triangles and a little beyond: equal distances to two triangles occur."""
    rng = np.random.default_rng(seed)
    rows = max(1, -(-T // 16))
    q = np.stack([rng.integers(-8, 16 * 16 + 8, n), rng.integers(-8, 16 * rows + 8, n), rng.integers(-4, 5, n)], axis=1)
    return (q / 8.0).astype(F32)


# ---------------------------------------------------------------- exact rational arithmetic ----------------------------------------------------------------
def _segment(p, a, b):
    ab = [y - x for x, y in zip(a, b)]
    ap = [y - x for x, y in zip(a, p)]
    L = sum(x * x for x in ab)
    t = Fraction(0) if L == 0 else max(Fraction(0), min(Fraction(1), sum(x * y for x, y in zip(ab, ap)) / L))
    return sum((pp - (aa + t * d)) ** 2 for pp, aa, d in zip(p, a, ab))


def exact_d2(p, a, b, c) -> Fraction:
    """The squared distance from p to the triangle a b c in rational arithmetic on the float32 inputs: the least of the three segments and,
    where the projection onto the plane falls inside the triangle, the distance to the plane."""
    p, a, b, c = ([Fraction(float(x)) for x in r] for r in (p, a, b, c))
    best = min(_segment(p, a, b), _segment(p, b, c), _segment(p, c, a))
    ab = [y - x for x, y in zip(a, b)]
    ac = [y - x for x, y in zip(a, c)]
    ap = [y - x for x, y in zip(a, p)]
    n = [ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]]
    nn = sum(x * x for x in n)
    if nn > 0:
        d00, d01, d11 = sum(x * x for x in ab), sum(x * y for x, y in zip(ab, ac)), sum(x * x for x in ac)
        d20, d21 = sum(x * y for x, y in zip(ap, ab)), sum(x * y for x, y in zip(ap, ac))
        den = d00 * d11 - d01 * d01
        v, w = (d11 * d20 - d01 * d21) / den, (d00 * d21 - d01 * d20) / den
        if v >= 0 and w >= 0 and v + w <= 1:
            h = sum(x * y for x, y in zip(n, ap))
            best = min(best, h * h / nn)
    return best


def _pair_kinds(n, seed):
    """kind -> (P, A, B, C) float32 [n, 3]: random triangles; slivers of height 1e-5; triangles of size 1e-4 at unit offset; queries 100 units away."""
    rng = np.random.default_rng(seed)
    u = lambda: rng.uniform(-1, 1, (n, 3))                                  # noqa: E731
    unit = lambda: (lambda d: d / np.linalg.norm(d, axis=1, keepdims=True))(rng.normal(size=(n, 3)))     # noqa: E731
    out = {"random": (u(), u(), u(), u())}
    A, B, t = u(), u(), rng.uniform(0, 1, (n, 1))
    out["sliver"] = (u(), A, B, A + t * (B - A) + 1e-5 * unit())
    O = u()
    O /= np.abs(O).max(axis=1, keepdims=True)
    out["tiny"] = (u(), O + 1e-4 * u(), O + 1e-4 * u(), O + 1e-4 * u())
    out["far"] = (100 * unit(), u(), u(), u())
    return {k: tuple(np.ascontiguousarray(x, dtype=F32) for x in val) for k, val in out.items()}


# ---------------------------------------------------------------- CPU: the oracle ----------------------------------------------------------------
def test_oracle_equals_exact_rational_arithmetic():
    """300 pairs of each kind, seed 0: the float64 d2 is within 2^-40 relative of the exact rational distance (measured: random 7.9e-15,
    sliver 1.3e-15, tiny 1.5e-16, far 2.3e-16, i.e. 2^-46.8 at worst), and the distance itself within 2^-48 of the largest coordinate.

    The relative cap is asserted for the pairs whose exact distance is at least 2^-8, and at least 295 of the 300 must be such.  X is
    placed in absolute coordinates, X = (A + AB v) + AC w, so it carries a rounding of about 2^-52 |X| and d2 a relative error of about
    2^-51 |X| / d whatever else is exact; with |X| <= sqrt(3), 2^-40 needs d >= 2^-10.  This draw holds one closer pair (random, 1.8e-5
    apart, 2^-39.5 relative); it is printed, and the absolute bound holds it like every other."""
    for kind, (P, A, B, C) in _pair_kinds(300, 0).items():
        d2, _, region = PO.closest_point(P, A, B, C)
        exact = [exact_d2(P[i], A[i], B[i], C[i]) for i in range(P.shape[0])]
        rel = [float(abs(Fraction(float(d2[i])) - ex) / ex) for i, ex in enumerate(exact)]
        apart = [i for i, ex in enumerate(exact) if ex >= Fraction(1, 2 ** 16)]
        worst = max(rel[i] for i in apart)
        worst_abs = max(abs(float(d2[i]) ** 0.5 - float(ex) ** 0.5) for i, ex in enumerate(exact))
        close = [(float(exact[i]) ** 0.5, rel[i]) for i in range(len(exact)) if i not in apart]
        print(f"{kind}: worst relative error of d2 {worst:.3e} = 2^{np.log2(worst):.1f} on {len(apart)} pairs at least 2^-8 apart; closer pairs (d, relative error): "
              f"{close}; worst absolute error of d {worst_abs:.3e}; regions {np.bincount(region, minlength=7).tolist()}")
        assert len(apart) >= 295, kind
        assert worst <= 2.0 ** -40, kind
        assert worst_abs <= 2.0 ** -48 * max(1.0, float(np.abs(P).max())), kind


# the triangle A = (0, 0, 0), B = (4, 0, 0), C = (0, 4, 0); every query's distance is a dyadic rational, so float64 states it exactly
REGION_QUERIES = [
    # strictly inside each region
    ((-1, -1, 1), "A"), ((5, -1, 1), "B"), ((2, -1, 1), "AB"), ((-1, 5, 1), "C"), ((-1, 2, 1), "AC"), ((3, 3, 1), "BC"), ((1, 1, 2), "interior"),
    # on the boundaries, where a test holds with equality: d1 == 0, d2 == 0, both (the vertex itself); d3 == 0, d4 == d3; vc == 0 (above the
    # edge AB, and on it); d6 == 0, d5 == d6; vb == 0 (above the edge AC); va == 0 (above the edge BC); the corners B and C themselves
    ((0, -1, 0), "A"), ((-1, 0, 0), "A"), ((0, 0, 0), "A"), ((0, 0, 3), "A"), ((4, -1, 0), "B"), ((5, 1, 0), "B"), ((4, 0, 0), "B"), ((2, 0, 1), "AB"),
    ((2, 0, 0), "AB"), ((-1, 4, 0), "C"), ((1, 5, 0), "C"), ((0, 4, 0), "C"), ((0, 2, 1), "AC"), ((2, 2, 1), "BC"), ((2, 2, 0), "BC"),
    ((1, 1, 0), "interior"),
]


def test_oracle_takes_every_region_and_boundary():
    A, B, Cc = (np.array(x, F32) for x in ((0, 0, 0), (4, 0, 0), (0, 4, 0)))
    P = np.array([p for p, _ in REGION_QUERIES], F32)
    n = P.shape[0]
    d2, X, region = PO.closest_point(P, np.tile(A, (n, 1)), np.tile(B, (n, 1)), np.tile(Cc, (n, 1)))
    assert [PO.REGIONS[r] for r in region] == [name for _, name in REGION_QUERIES]
    assert set(region.tolist()) == set(range(7))                            # every branch is taken
    for i in range(n):
        assert Fraction(float(d2[i])) == exact_d2(P[i], A, B, Cc), REGION_QUERIES[i]
        assert sum((Fraction(float(P[i, k])) - Fraction(float(X[i, k]))) ** 2 for k in range(3)) == exact_d2(P[i], A, B, Cc)
    # the same through the search, as a one-triangle mesh and under every rotation of its corners: the distance does not depend on which
    # corner is called A
    v = np.stack([A, B, Cc])
    for f in ([0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 2, 1]):
        got_d2, got_tri, got_pt = PO.nearest_on_mesh(P, v, np.array([f], np.int32))
        assert got_d2.tobytes() == d2.astype(F32).tobytes() and (got_tri == 0).all() and got_pt.tobytes() == X.astype(F32).tobytes()


def test_oracle_validity_on_the_hostile_mesh():
    """Only triangles 0, 5 and 7 are valid.  Triangle 5 has w = 2^-34 > 0: it IS valid here, though the sampler never draws it (its integer
    weight floor(2^-34 2^32) is 0) -- a surface too small to be sampled is still a surface a point can be close to."""
    v, f = _hostile_mesh()
    assert np.flatnonzero(PO.valid_triangles(v, f)).tolist() == list(HOSTILE_VALID)
    assert MO.face_normals(v, f)[1][5] == 2.0 ** -34 and MO.integer_weights(v, f)[5] == 0
    q = _hostile_queries()
    d2, tri, pt = PO.nearest_on_mesh(q, v, f)
    assert tri[:7].tolist() == [0, 5, 7, 5, 5, 0, 0]                        # (0, 0, 0.5) is as far from 0 as from 7: the lower index
    assert d2[6] == F32(0.25) and d2[1] == F32(0.25) and pt[1].tolist() == [5, 5, 5]
    assert set(tri.tolist()) <= set(HOSTILE_VALID) | {-1}
    for i in (7, 8, 9):                                                     # a NaN coordinate: every pair is NaN
        assert np.isposinf(d2[i]) and tri[i] == -1 and np.isnan(pt[i]).all()
    for i in range(7):                                                      # all-pairs by hand over the valid triangles only
        want = min((F32(float(PO.closest_point(q[i], *v[f[t]])[0])), t) for t in HOSTILE_VALID)
        assert (d2[i], tri[i]) == want
    # +inf is an ordinary value: 3e38 away the float64 distance overflows float32, and the lowest valid triangle holds it; 1e18 away it does not
    assert np.isposinf(d2[12]) and tri[12] == 0 and np.isfinite(d2[13]) and tri[13] in HOSTILE_VALID
    # no valid triangle at all is not an error
    d2, tri, pt = PO.nearest_on_mesh(q, v, f[[1, 2, 3, 4, 6, 8]])
    assert np.isposinf(d2).all() and (tri == -1).all() and np.isnan(pt).all()
    d2, tri, pt = PO.nearest_on_mesh(q, v[:0], f)
    assert np.isposinf(d2).all() and (tri == -1).all() and np.isnan(pt).all()


# ---------------------------------------------------------------- CPU: plumbing and argument checks ----------------------------------------------------------------
def test_build_lists_signatures_and_defaults():
    assert {"pointmesh_kernels.hip", "pointmesh_capi.cpp"} <= set(_build.SOURCES) and {"pointmesh.h", "mesh_triangle.h"} <= set(_build.HEADERS)
    assert _build.SOURCE_FLAGS["pointmesh_kernels.hip"] == ["-ffp-contract=off"]
    for name in ("pointmesh_kernels.hip", "pointmesh_capi.cpp", "pointmesh.h", "mesh_triangle.h"):
        assert os.path.exists(os.path.join(_build.CSRC, name))
    assert {"tsamd_nearest_on_mesh", "tsamd_nearest_on_mesh_workspace_bytes", "tsamd_nearest_on_mesh_info"} <= set(_capi.SIGNATURES)
    assert _capi.ABI_VERSION == 3 and _capi.load().tsamd_abi_version() == 3   # an addition is no incompatible change
    from tssplat_amd import geometry, metrics
    assert {"nearest_on_mesh", "nearest_on_mesh_info", "compare_meshes_exact", "NearestOnMeshInfo"} <= set(metrics.__all__)
    sig = inspect.signature(metrics.nearest_on_mesh).parameters
    assert sig["ref_chunks"].default == 0 and sig["return_points"].default is True
    sig = inspect.signature(metrics.compare_meshes_exact).parameters
    assert (sig["n"].default, sig["seed"].default, sig["thresholds"].default) == (100_000, 0, (0.01, 0.02))
    assert inspect.signature(geometry.TetMeshGeometry.surface_metrics).parameters["exact"].default is False
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import lab_variants
        import train_object
    finally:
        sys.path.pop(0)
    assert inspect.signature(train_object.run).parameters["eval_exact"].default is False
    assert '"--eval-exact", action="store_true"' in inspect.getsource(train_object.main)
    for name in ("pointmesh_noprune", "pointmesh_q2", "pointmesh_q4", "pointmesh_tile256", "pointmesh_count"):
        assert lab_variants.patched_sources(name)                           # every anchor is still in its file


def test_nearest_on_mesh_info_reports_the_compiled_constants():
    from tssplat_amd import metrics
    info = metrics.nearest_on_mesh_info(100_000, 100_000)
    assert info.block % 64 == 0 and info.queries_per_lane >= 1 and info.tri_tile % 8 == 0 and info.tri_tile * 16 <= 64 * 1024
    per = info.block * info.queries_per_lane
    assert 1 <= info.auto_chunks <= -(-100_000 // info.tri_tile)
    assert metrics.nearest_on_mesh_info(1, 1).auto_chunks == 1 and metrics.nearest_on_mesh_info(0, 0).auto_chunks == 1
    assert metrics.nearest_on_mesh_info(1, 10 * info.tri_tile).auto_chunks == 10               # one query block: a chunk is never less than a tile
    assert metrics.nearest_on_mesh_info(10_000 * per, 10 * info.tri_tile).auto_chunks == 1     # enough query blocks on their own
    with pytest.raises(RuntimeError, match="n must be"):
        metrics.nearest_on_mesh_info(-1, 4)
    with pytest.raises(RuntimeError, match="t must be"):
        metrics.nearest_on_mesh_info(4, 2 ** 31)
    lib = _capi.load()
    size = lib.tsamd_nearest_on_mesh_workspace_bytes
    assert size(0, 0) == 0 and size(1, 1) > 0 and size(1, 1) % 16 == 0 and size(7, 5) % 16 == 0
    assert size(1000, 10) > size(10, 10) and size(10, 1000) > size(10, 10) and size(2 ** 31 - 1, 2 ** 31 - 1) > 2 ** 31
    assert size(-1, 1) == -1 and size(1, -1) == -1 and size(2 ** 31, 1) == -1 and size(1, 2 ** 31) == -1


def test_c_abi_argument_errors_launch_nothing():
    """Every argument error is reported before anything touches the device: all device pointers here are null or made up."""
    lib = _capi.load()
    p = 0x1000                                                              # "not null", aligned; never dereferenced on these paths
    odd, half = 0x1002, 0x1008                                              # not 4-byte, not 16-byte aligned

    def near(q=p, n=4, v=p, nv=3, f=p, nt=4, chunks=0, work=p, d2=p, tri=p, pt=p):
        return lib.tsamd_nearest_on_mesh(q, n, v, nv, f, nt, chunks, work, d2, tri, pt, None)

    def info(n=4, nt=4, out=(1, 1, 1, 1)):
        slots = [C.c_int32() for _ in range(4)]
        return lib.tsamd_nearest_on_mesh_info(n, nt, *(C.byref(s) if keep else None for s, keep in zip(slots, out)))

    big = 2 ** 31
    cases = [
        (near, dict(n=-1), "n out"), (near, dict(n=big), "n out"), (near, dict(nt=0), "n_triangles"), (near, dict(nt=-3), "n_triangles"),
        (near, dict(nt=big), "n_triangles"), (near, dict(nv=-1), "n_vertices"), (near, dict(nv=big), "n_vertices"),
        (near, dict(chunks=-1), "ref_chunks"), (near, dict(chunks=5), "ref_chunks"), (near, dict(nt=70000, chunks=65536), "ref_chunks"),
        (near, dict(q=None), "query_dev"), (near, dict(v=None), "v_dev"), (near, dict(f=None), "faces_dev"), (near, dict(work=None), "workspace_dev"),
        (near, dict(d2=None), "d2_out_dev"), (near, dict(tri=None), "tri_out_dev"), (near, dict(q=odd), "query_dev"), (near, dict(v=odd), "v_dev"),
        (near, dict(f=odd), "faces_dev"), (near, dict(work=half), "workspace_dev"), (near, dict(d2=odd), "d2_out_dev"), (near, dict(tri=odd), "tri_out_dev"),
        (near, dict(pt=odd), "point_out_dev"),
        (info, dict(n=-1), "n out"), (info, dict(nt=big), "n_triangles"), (info, dict(out=(0, 1, 1, 1)), "block_out"),
        (info, dict(out=(1, 0, 1, 1)), "queries_per_lane_out"), (info, dict(out=(1, 1, 0, 1)), "tri_tile_out"), (info, dict(out=(1, 1, 1, 0)), "auto_chunks_out"),
    ]
    for fn, kw, word in cases:
        assert fn(**kw) == INVALID, (fn.__name__, kw)
        msg = lib.tsamd_last_error().decode()
        assert msg and word in msg, (fn.__name__, kw, msg)
    # nothing to do is not an error, and still launches nothing: no queries
    assert near(n=0, q=None, work=None, d2=None, tri=None, pt=None) == 0
    assert info() == 0 and info(n=0, nt=0) == 0                             # the query touches no device
    assert _capi.ABI_VERSION == 3 and lib.tsamd_abi_version() == 3


def test_python_arguments_are_checked_by_name():
    """Nothing here reaches the library: a CPU tensor is refused first, with the argument's name."""
    from tssplat_amd import metrics
    v, f, pts = torch.zeros(4, 3), torch.zeros(1, 3, dtype=torch.int32), torch.zeros(5, 3)
    for call, word in [(lambda: metrics.nearest_on_mesh(pts, v, f), "query must be a GPU tensor"), (lambda: metrics.nearest_on_mesh(None, v, f), "query must"),
                       (lambda: metrics.compare_meshes_exact(v, f, v, f, n=0), "n must be"), (lambda: metrics.compare_meshes_exact(v, f, v, f, n=10), "v_a must"),
                       (lambda: metrics.compare_meshes_exact(v, f, v, f, thresholds=(-1.0,)), "thresholds must"),
                       (lambda: metrics.compare_meshes_exact(v, f, v, f, seed=0.5), "seed must")]:
        with pytest.raises(RuntimeError, match=word):
            call()


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"), reason="needs the ROCm LLVM tools")
def test_kernels_are_in_the_code_object_and_do_not_spill():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_metadata
    finally:
        sys.path.pop(0)
    _capi.load()
    meta = kernel_metadata.kernel_metadata(_capi.lib_path())
    for want in ("pointmesh_prepare_kernel", "pointmesh_seed_kernel", "pointmesh_search_kernel", "pointmesh_finish_kernel"):
        recs = [v for k, v in meta.items() if want in k]
        assert len(recs) == 1, want
        assert recs[0]["vgpr_spill_count"] == 0 and recs[0]["private_segment_fixed_size"] == 0, (want, recs[0])


# ---------------------------------------------------------------- GPU: against the oracle, bit for bit ----------------------------------------------------------------
def _info():
    from tssplat_amd import metrics
    return metrics.nearest_on_mesh_info(1, 1)


def _assert_bits(got, want, what):
    d2, tri, pt = (x.cpu().numpy() for x in got)
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32 and got[2].dtype == torch.float32
    assert tri.tobytes() == want[1].tobytes(), (what, "tri", int((tri != want[1]).sum()), np.flatnonzero(tri != want[1])[:8].tolist())
    assert d2.tobytes() == want[0].tobytes(), (what, "d2", int((d2.view(np.uint32) != want[0].view(np.uint32)).sum()))
    assert pt.tobytes() == want[2].tobytes(), (what, "point", int((pt.view(np.uint32) != want[2].view(np.uint32)).sum()))


def _chunk_counts(T):
    return sorted({c for c in (1, 2, 7, min(T, 65535)) if c <= T}) + [0]


def _search_all_chunks(q, v, f, want, what):
    from tssplat_amd import metrics
    qd, vd, fd = dev(q), dev(v), dev(f)
    for chunks in _chunk_counts(f.shape[0]):
        _assert_bits(metrics.nearest_on_mesh(qd, vd, fd, ref_chunks=chunks), want, (what, chunks))


@gpu
@pytest.mark.parametrize("which", ["1", "K-1", "K", "K+1", "2K+1"])
def test_query_and_tile_edges_equal_oracle_for_every_chunk_count(which):
    info = _info()
    Q, K = info.block * info.queries_per_lane, info.tri_tile
    T = {"1": 1, "K-1": K - 1, "K": K, "K+1": K + 1, "2K+1": 2 * K + 1}[which]
    v, f = _lattice_mesh(T)
    q = _lattice_queries(2 * Q + 1, T, seed=T)
    want = PO.nearest_on_mesh(q, v, f)                                      # per query: a prefix of the queries has a prefix of the results
    assert T == 1 or len(set(want[1].tolist())) > 1
    for N in (1, Q - 1, Q, Q + 1, 2 * Q + 1):
        _search_all_chunks(q[:N], v, f, tuple(x[:N] for x in want), (which, N))


GOLDEN_SAMPLES = 768


@functools.lru_cache(maxsize=None)
def _golden_case(name):
    """(queries, parts, oracle results): surface samples, the first 256 vertices, the mesh's centre, the samples scaled by 1e3 (against the mesh
    scaled by 1e3, searched separately)."""
    v, f = _golden(name)
    s = MO.sample_surface(v, f, GOLDEN_SAMPLES, 11).points
    centre = (0.5 * (v.min(axis=0).astype(np.float64) + v.max(axis=0))).astype(F32)[None]
    q = np.concatenate([s, v[:256], centre])
    parts = {"samples": slice(0, GOLDEN_SAMPLES), "vertices": slice(GOLDEN_SAMPLES, GOLDEN_SAMPLES + 256), "centre": slice(GOLDEN_SAMPLES + 256, None)}
    return q, parts, PO.nearest_on_mesh(q, v, f)


@gpu
@pytest.mark.parametrize("name", ["s1_sphere", "mario_mesh"])
def test_golden_meshes_equal_oracle(name):
    from tssplat_amd import metrics
    v, f = _golden(name)
    q, parts, want = _golden_case(name)
    d2, tri, pt = want
    # what the oracle says about these queries (CPU preconditions of the device checks below)
    s = parts["samples"]
    own = MO.sample_surface(v, f, GOLDEN_SAMPLES, 11).tri
    assert (np.sqrt(d2[s].astype(np.float64)) < 1e-6).all() and (tri[s] == own).all()          # every sample finds its own triangle
    vs = parts["vertices"]
    assert (d2[vs] == 0).all()
    first_incident = np.array([np.flatnonzero((f == i).any(axis=1))[0] for i in range(256)])
    assert (tri[vs] == first_incident).all()                                # about six incident triangles tie at 0: the lowest index wins
    _assert_bits(metrics.nearest_on_mesh(dev(q), dev(v), dev(f)), want, name)
    got = metrics.nearest_on_mesh(dev(q), dev(v), dev(f), ref_chunks=3, return_points=False)
    assert got[2] is None and got[0].cpu().numpy().tobytes() == d2.tobytes() and got[1].cpu().numpy().tobytes() == tri.tobytes()


@gpu
@pytest.mark.parametrize("name", ["s1_sphere", "mario_mesh"])
def test_golden_meshes_scaled_by_1000_equal_oracle(name):
    """Mesh and queries a thousand times larger: the sphere test's margin is relative, and the float32 radius and centre round coarser.  Then
    the scaled queries against the mesh as it is: a thousand mesh sizes away, where every triangle is nearly equidistant."""
    from tssplat_amd import metrics
    v, f = _golden(name)
    q = _golden_case(name)[0]
    big_v, big_q = v * F32(1000), q[::2] * F32(1000)
    want = PO.nearest_on_mesh(big_q, big_v, f)
    _assert_bits(metrics.nearest_on_mesh(dev(big_q), dev(big_v), dev(f)), want, "both scaled")
    far = PO.nearest_on_mesh(big_q[:256], v, f)
    _assert_bits(metrics.nearest_on_mesh(dev(big_q[:256]), dev(v), dev(f), ref_chunks=2), far, "queries scaled")


@gpu
def test_ties_across_tiles_and_chunks_go_to_the_lowest_index():
    info = _info()
    K = info.tri_tile
    T = 2 * K + 1
    v, f = _lattice_mesh(T)
    near = f[K + 7].copy()                                                  # one triangle, four times in the mesh
    for at in (0, K - 1, K, T - 1):
        f[at] = near
    q = (v[near].mean(axis=0) + np.array([[0, 0, 0.25], [0.125, 0, 0], [0.25, 0.5, 0]], F32)).astype(F32)
    want = PO.nearest_on_mesh(q, v, f)
    assert want[1].tolist() == [0, 0, 0]
    _search_all_chunks(q, v, f, want, "four copies")
    f[0] = [0, -1, 2]                                                       # the copy at index 0 made invalid: the next one wins
    want = PO.nearest_on_mesh(q, v, f)
    assert want[1].tolist() == [K - 1, K - 1, K - 1]
    _search_all_chunks(q, v, f, want, "first copy invalid")


@gpu
def test_a_huge_triangle_with_a_far_centre_is_not_pruned():
    """The pruning trap: the query hovers 1e-3 above a triangle with edges of 1e3 whose centre is hundreds of units away, beside 2 048 small
    triangles whose centres are all closer than that and whose surfaces are all farther than 1e-3."""
    small_v, small_f = _lattice_mesh(2048)
    small_v = small_v + np.array([0, 0, 5], F32)
    huge_v = np.array([[-10, -10, 0], [990, -10, 0], [-10, 990, 0]], F32)
    v = np.concatenate([small_v, huge_v])
    f = np.concatenate([small_f, [[small_v.shape[0], small_v.shape[0] + 1, small_v.shape[0] + 2]]]).astype(np.int32)
    q = np.array([[10, 10, 1e-3], [3.25, 7.5, 1e-3], [20, 100, 2.5], [20, 100, 2.625], [5, 5, 4.5]], F32)
    want = PO.nearest_on_mesh(q, v, f)
    centre = huge_v.mean(axis=0)
    assert (np.linalg.norm(q - centre, axis=1) > 300).all() and want[1].tolist()[:2] == [2048, 2048] and abs(float(want[0][0]) - 1e-6) < 1e-12
    assert want[0][2] == F32(6.25) and want[1][2] == want[1][3] < 2048 and want[1][4] < 2048           # a tie with a small triangle: the lower index
    _search_all_chunks(q, v, f, want, "huge")
    first = PO.nearest_on_mesh(q, v, f[::-1])
    assert first[1].tolist()[:3] == [0, 0, 0]                               # ... which is the huge one when it comes first
    _search_all_chunks(q, v, np.ascontiguousarray(f[::-1]), first, "huge first")


@gpu
def test_invalid_inputs_on_the_device():
    from tssplat_amd import metrics
    v, f = _hostile_mesh()
    q = _hostile_queries()
    want = PO.nearest_on_mesh(q, v, f)
    _search_all_chunks(q, v, f, want, "hostile")
    qd, vd, fd = dev(q), dev(v), dev(f)
    once, again = metrics.nearest_on_mesh(qd, vd, fd), metrics.nearest_on_mesh(qd, vd, fd)
    for a, b in zip(once, again):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()      # bitwise repeatable
    # a mesh with no valid triangle is not an error
    for vv, ff in ((v, f[[1, 2, 3, 4, 6, 8]]), (v[:0], f)):
        got = metrics.nearest_on_mesh(qd, dev(vv), dev(np.ascontiguousarray(ff)))
        _assert_bits(got, PO.nearest_on_mesh(q, vv, ff), "no valid triangle")
        assert torch.isposinf(got[0]).all() and (got[1] == -1).all() and torch.isnan(got[2]).all()
    for call, word in [(lambda: metrics.nearest_on_mesh(qd, vd, fd[:0]), "faces holds no triangle"), (lambda: metrics.nearest_on_mesh(qd, vd, fd, ref_chunks=10), "ref_chunks must"),
                       (lambda: metrics.nearest_on_mesh(qd, vd, fd, ref_chunks=-1), "ref_chunks must"), (lambda: metrics.nearest_on_mesh(qd.double(), vd, fd), "query must be float32"),
                       (lambda: metrics.nearest_on_mesh(qd, vd, fd.long()), "faces must be int32"), (lambda: metrics.nearest_on_mesh(qd, vd.cpu(), fd), "v must be a GPU"),
                       (lambda: metrics.nearest_on_mesh(qd, vd, fd, return_points=1), "return_points must")]:
        with pytest.raises(RuntimeError, match=word):
            call()
    d2, tri, pt = metrics.nearest_on_mesh(qd[:0], vd, fd)                   # N == 0: empty tensors
    assert tuple(d2.shape) == (0,) and tuple(tri.shape) == (0,) and tuple(pt.shape) == (0, 3)


# ---------------------------------------------------------------- GPU: the metrics on top ----------------------------------------------------------------
FLOAT_FIELDS = ("chamfer_l1", "chamfer_l2", "accuracy", "completeness", "accuracy_max", "completeness_max", "normal_consistency")


def _oracle_compare_exact(v_a, f_a, v_b, f_b, n, seed, thresholds=(0.01, 0.02)):
    """compare_meshes_exact in numpy: the sampler's samples, the oracle's d2 / tri, metrics_oracle's float64 reductions, and the unit normal
    of the winning triangle where compare has the nearest sample's."""
    def unit(v, f):
        nrm, w, _ = MO.face_normals(v, f)
        with np.errstate(invalid="ignore", divide="ignore"):
            return nrm / w[:, None]
    a, b, b2 = MO.sample_surface(v_a, f_a, n, seed + 2), MO.sample_surface(v_b, f_b, n, seed), MO.sample_surface(v_b, f_b, n, seed + 1)
    d2_ab, tri_ab, _ = PO.nearest_on_mesh(a.points, v_b, f_b)
    d2_ba, tri_ba, _ = PO.nearest_on_mesh(b.points, v_a, f_a)
    d2_fl, tri_fl, _ = PO.nearest_on_mesh(b2.points, v_b, f_b)
    ab = MO._one_side(d2_ab, tri_ab, a.normals, unit(v_b, f_b), thresholds)
    ba = MO._one_side(d2_ba, tri_ba, b.normals, unit(v_a, f_a), thresholds)
    rec = {"n_a": n, "n_b": n, "chamfer_l1": 0.5 * (ab.mean + ba.mean), "chamfer_l2": ab.mean_sq + ba.mean_sq, "accuracy": ab.mean, "completeness": ba.mean,
           "accuracy_max": ab.max, "completeness_max": ba.max, "normal_consistency": 0.5 * (ab.normal + ba.normal),
           "dropped_ab": ab.dropped, "dropped_ba": ba.dropped, "thresholds": [],
           "noise_floor": MO._one_side(d2_fl, tri_fl, b2.normals, unit(v_b, f_b), thresholds).mean}
    for k, t in enumerate(thresholds):
        P, R = ab.counts[k] / n, ba.counts[k] / n
        rec["thresholds"].append({"tau": float(t), "precision": P, "recall": R, "fscore": 2 * P * R / (P + R) if P + R > 0 else 0.0,
                                  "precision_count": ab.counts[k], "recall_count": ba.counts[k]})
    return rec


def _assert_record_close(got, want, n):
    """The bound of tests/test_metrics.py's _assert_record_close, restated.  Integers equal; floats within the rounding of a float64 mean of n
    float32 square roots: d2 and tri are the oracle's bits, so only the square root (the device's within one ulp, 2 U of d; numpy's correctly
    rounded, U) and the order of the float64 sums (n U64 relative on sums of non-negative terms, each side) differ:
    |mean - mean'| <= (3 U32 + 2 n U64) mean.  chamfer_l2 has no root: 2 n U64.  normal_consistency: (2 n + 4) U64 -- the winning triangle's
    unit normal is the same float64 operations in torch and in numpy, each cosine three products and two sums after it."""
    g = got.as_dict()
    for key in ("n_a", "n_b", "dropped_ab", "dropped_ba"):
        assert g[key] == want[key], key
    for tg, tw in zip(g["thresholds"], want["thresholds"]):
        assert (tg["precision_count"], tg["recall_count"], tg["tau"]) == (tw["precision_count"], tw["recall_count"], tw["tau"])
        for key in ("precision", "recall", "fscore"):
            assert tg[key] == tw[key], key
    rel = {"chamfer_l2": 2 * n * U64, "normal_consistency": (2 * n + 4) * U64}
    for key in FLOAT_FIELDS + ("noise_floor",):
        bound = rel.get(key, 3 * U32 + 2 * n * U64) * abs(want[key])
        print(f"{key}: {g[key]!r} oracle {want[key]!r} |diff| {abs(g[key] - want[key]):.3e} bound {bound:.3e}")
        assert abs(g[key] - want[key]) <= bound, key


@gpu
def test_compare_meshes_exact_of_a_mesh_against_itself_has_no_floor():
    """Samples of a mesh lie on the mesh up to the rounding of the sampler's float32 point: accuracy, completeness and noise_floor are below
    1e-6 of the bounding-box diagonal (the oracle's largest d on the unit sphere is 7.5e-8), where the sampled comparison stays at its floor."""
    from tssplat_amd import metrics
    v, f = _golden("s1_sphere")
    diag = float(np.linalg.norm(v.max(axis=0).astype(np.float64) - v.min(axis=0)))
    vd, fd = dev(v), dev(f)
    n = 4096
    exact, sampled = metrics.compare_meshes_exact(vd, fd, vd, fd, n=n, seed=0), metrics.compare_meshes(vd, fd, vd, fd, n=n, seed=0)
    print(f"exact: accuracy {exact.accuracy:.3e} completeness {exact.completeness:.3e} noise_floor {exact.noise_floor:.3e} max {exact.accuracy_max:.3e}; "
          f"sampled: chamfer_l1 {sampled.chamfer_l1:.3e} noise_floor {sampled.noise_floor:.3e}; diagonal {diag:.3f}")
    assert 0 <= exact.accuracy < 1e-6 * diag and 0 <= exact.completeness < 1e-6 * diag and 0 <= exact.noise_floor < 1e-6 * diag
    assert exact.n_a == exact.n_b == n and exact.dropped_ab == exact.dropped_ba == 0 and exact.thresholds[0].fscore == 1.0
    assert exact.normal_consistency > 1 - 1e-6
    assert sampled.chamfer_l1 > exact.chamfer_l1 and sampled.accuracy > exact.accuracy and sampled.completeness > exact.completeness
    assert metrics.compare_meshes_exact(vd, fd, vd, fd, n=n, seed=0).as_dict() == exact.as_dict()       # bit for bit


@gpu
def test_compare_meshes_exact_equals_the_oracle_reductions():
    from tssplat_amd import geometry, metrics, scenes
    v, f = _golden("s1_sphere")
    big = v * F32(1.05)
    n, taus = 1024, (0.04, 0.04985, 0.2)                                   # the middle one cuts through the samples
    got = metrics.compare_meshes_exact(dev(big), dev(f), dev(v), dev(f), n=n, seed=4, thresholds=taus)
    want = _oracle_compare_exact(big, f, v, f, n, 4, taus)
    _assert_record_close(got, want, n)
    assert 0.04 < got.accuracy < 0.06 and 0 < got.thresholds[1].precision_count < n
    # the geometry's keyword is compare_meshes_exact of its boundary
    bv, bt = scenes.kuhn_ball(4)
    bv = (bv / np.linalg.norm(bv, axis=1).max()).astype(F32)
    geo = geometry.TetMeshGeometry(bv, bt.astype(np.int32), use_smooth_barrier=False)
    mine = geo.surface_metrics(dev(v), dev(f), n=512, seed=3, exact=True)
    ref = metrics.compare_meshes_exact(geo.tet_v.detach()[geo.surface_vid.long()].contiguous(), geo.surface_fid, dev(v), dev(f), n=512, seed=3)
    assert mine.as_dict() == ref.as_dict() and mine.noise_floor < 1e-6 and mine.chamfer_l1 < 0.2
