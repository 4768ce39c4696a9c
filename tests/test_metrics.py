"""Surface metrics (tssplat_amd/metrics.py: sample_surface, nearest, compare, compare_meshes).  The sampler and the nearest-point
search are integers and separately rounded operations: the device results are compared with tests/metrics_oracle.py bit for bit.
The oracle itself is checked on the CPU: the sampler against the area law (chi-square) and its edge cases, the float32 search
against a float64 brute force wherever float64 separates the winner from the runner-up, the metrics on two concentric spheres."""
import ctypes as C
import functools
import inspect
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import metrics_oracle as MO
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


def _decades_mesh(T=40):
    """T isolated right triangles in the plane z = 0 whose areas run log-spaced over three decades."""
    area = np.logspace(0, 3, T)
    leg = np.sqrt(2 * area).astype(F32)
    v = np.zeros((T, 3, 3), F32)
    v[:, :, 0] = 100.0 * np.arange(T)[:, None]
    v[:, 1, 0] += leg
    v[:, 2, 1] = leg
    return v.reshape(-1, 3), np.arange(3 * T, dtype=np.int32).reshape(T, 3)


def _hostile_mesh():
    """Triangle 0: area 1/2 (w = 1).  1: zero area (repeated corner).  2: a NaN vertex.  3: an index past the end.  4: a negative index.
    5: w = 2^-34, so q = floor(2^-34 2^32) = 0.  6: collinear corners.  7: area 1/8 (w = 1/4).  8: an infinite vertex."""
    s = 2.0 ** -17
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [5, 5, 5], [5 + s, 5, 5], [5, 5 + s, 5], [2, 2, 2], [3, 3, 3], [4, 4, 4],
                  [0, 0, 1], [0.5, 0, 1], [0, 0.5, 1], [np.inf, 0, 0]], F32)
    f = np.array([[0, 1, 2], [0, 1, 1], [0, 3, 2], [0, 1, 14], [0, -1, 2], [4, 5, 6], [7, 8, 9], [10, 11, 12], [0, 13, 2]], np.int32)
    return v, f


DRAWABLE = (0, 7)           # the triangles of _hostile_mesh with q > 0


def _one_triangle():
    return np.array([[0.25, -1, 3], [2, 0.5, 3.5], [-1, 1.5, 2]], F32), np.array([[0, 1, 2]], np.int32)


MESHES = {"s1_sphere": lambda: _golden("s1_sphere"), "mario": lambda: _golden("mario_mesh"), "hostile": _hostile_mesh, "one_triangle": _one_triangle}


@functools.lru_cache(maxsize=None)
def _oracle_samples(mesh, n, seed):
    return MO.sample_surface(*MESHES[mesh](), n, seed)


# ---------------------------------------------------------------- CPU: the sampler ----------------------------------------------------------------
def test_mix64_is_the_splitmix64_stream():
    """mix64(seed, c) is output c of splitmix64 started at `seed`: the published first outputs for seed 0."""
    assert [MO.mix64(0, c) for c in range(3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    c = np.arange(1000, dtype=np.uint64)
    assert MO.mix64_array(12345, c).tolist() == [MO.mix64(12345, int(x)) for x in c]
    assert MO.mix64_array(2 ** 64 - 1, c[:5]).tolist() == [MO.mix64(2 ** 64 - 1, int(x)) for x in c[:5]]


def test_sampler_area_law_chi_square():
    """2 x 10^5 draws over 40 triangles whose areas span three decades: the per-triangle counts against n q / Q.  Level 10^-3 (the
    fixed seed either passes or it does not; a wrong weighting or search misses by orders of magnitude)."""
    from scipy import stats
    v, f = _decades_mesh()
    n = 200_000
    s = MO.sample_surface(v, f, n, seed=7)
    q = np.array([int(x) for x in s.q], dtype=np.float64)
    area = 0.5 * np.linalg.norm(np.cross(v[f[:, 1]].astype(np.float64) - v[f[:, 0]], v[f[:, 2]].astype(np.float64) - v[f[:, 0]]), axis=1)
    assert area.max() / area.min() > 999 and np.allclose(q / q.sum(), area / area.sum(), rtol=0, atol=2.0 ** -31)
    expected = n * q / q.sum()
    assert expected.min() > 5
    observed = np.bincount(s.tri, minlength=f.shape[0])
    chi2 = float(((observed - expected) ** 2 / expected).sum())
    limit = float(stats.chi2.ppf(1 - 1e-3, f.shape[0] - 1))
    print(f"chi2 {chi2:.2f} limit {limit:.2f} (df {f.shape[0] - 1})")
    assert chi2 < limit
    # and within a triangle: the barycentrics are uniform, so a + b < 1/2 holds for a quarter of the samples
    inner = int((s.a.astype(np.float64) + s.b < 0.5).sum())
    assert abs(inner - n / 4) < 4.5 * np.sqrt(n * 0.25 * 0.75)


def test_sampler_edge_cases():
    v, f = _hostile_mesh()
    s = MO.sample_surface(v, f, 20_000, seed=3)
    assert [int(x) for x in s.q] == [2 ** 32, 0, 0, 0, 0, 0, 0, 2 ** 30, 0]
    assert set(np.unique(s.tri).tolist()) == set(DRAWABLE)                   # zero-area, NaN, bad-index and q = 0 triangles are never drawn
    assert abs(int((s.tri == 7).sum()) - 4000) < 4.5 * np.sqrt(20_000 * 0.2 * 0.8)
    a, b = s.a.astype(np.float64), s.b.astype(np.float64)
    assert a.min() >= 0 and b.min() >= 0 and (a + b).max() <= 1.0           # the closed triangle, exactly
    assert np.isfinite(s.points).all() and np.allclose(np.linalg.norm(s.normals.astype(np.float64), axis=1), 1, atol=4 * U32)
    assert (s.points[s.tri == 0][:, 2] == 0).all() and (s.points[s.tri == 7][:, 2] == 1).all()
    # a single triangle: every sample lies in its plane, inside it
    v1, f1 = _one_triangle()
    s1 = MO.sample_surface(v1, f1, 500, seed=0)
    assert (s1.tri == 0).all() and s1.Q == 2 ** 32
    A, B, Cc = (v1[k].astype(np.float64) for k in range(3))
    want = A + s1.a.astype(np.float64)[:, None] * (B - A) + s1.b.astype(np.float64)[:, None] * (Cc - A)
    assert np.abs(s1.points - want).max() <= 16 * U32 * np.abs(v1).max()
    # the draws are counter-based: sample i does not depend on n
    assert MO.sample_surface(v1, f1, 7, seed=0).points.tobytes() == s1.points[:7].tobytes()
    assert MO.sample_surface(v1, f1, 0, seed=0).points.shape == (0, 3)
    # Q == 0
    for vv, ff in [(v, f[[1, 2, 3, 4, 6, 8]]), (v, f[:0]), (v[:0], f[:1])]:
        with pytest.raises(RuntimeError, match="faces"):
            MO.sample_surface(vv, ff, 4, seed=0)


# ---------------------------------------------------------------- CPU: nearest ----------------------------------------------------------------
def test_oracle_nearest_agrees_with_float64_where_float64_decides():
    """The form's float32 rounding: dx carries U, dx^2 3 U, the first sum 4 U, the second 5 U -- |d2_32 - d2_64| <= 6 U d2 with the
    second order.  Where the float64 minimum and the runner-up are further apart than both bounds, float32 must pick the same row."""
    rng = np.random.default_rng(11)
    q, r = rng.uniform(-1, 1, (2000, 3)).astype(F32), rng.uniform(-1, 1, (3000, 3)).astype(F32)
    d2, idx = MO.nearest(q, r)
    lo, arg, second = MO.nearest_f64(q, r)
    assert (np.abs(d2.astype(np.float64) - lo) <= 6 * U32 * lo).all()        # the minimum's value holds with or without separation
    decided = second - lo > 6 * U32 * (second + lo)
    excluded = 1.0 - decided.mean()
    print(f"excluded share {excluded:.2e}")
    assert excluded < 0.01
    assert (idx[decided] == arg[decided]).all()


def test_oracle_nearest_ties_nans_and_infinities():
    lattice = np.stack(np.meshgrid(*[np.arange(5)] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(F32)
    centres = (np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), axis=-1).reshape(-1, 3) + 0.5).astype(F32)
    faces = centres.copy()
    faces[:, 2] -= 0.5
    for q, ties, value in ((centres, 8, 0.75), (faces, 4, 0.5)):
        d2_all = ((q[:, None, :] - lattice[None, :, :]) ** 2).sum(axis=2)
        assert ((d2_all == d2_all.min(axis=1, keepdims=True)).sum(axis=1) == ties).all()      # exactly tied, in float32
        d2, idx = MO.nearest(q, lattice)
        assert (d2 == value).all() and (idx == (d2_all == value).argmax(axis=1)).all()        # the lowest index
        assert (MO.nearest(q, np.concatenate([lattice, lattice]))[1] == idx).all()            # duplicated ref points
    nan, inf = np.nan, np.inf
    d2, idx = MO.nearest(np.array([[0, 0, 0], [nan, 0, 0], [inf, 0, 0]], F32), np.array([[nan, 1, 1], [-inf, 0, 0], [inf, 0, 0], [3, 0, 0]], F32))
    assert idx.tolist() == [3, -1, 1] and d2.tolist() == [9.0, inf, inf]                      # inf - inf is a NaN: row 2 of ref is skipped
    assert MO.nearest(np.zeros((2, 3), F32), np.full((3, 3), nan, F32))[1].tolist() == [-1, -1]
    with pytest.raises(RuntimeError, match="ref"):
        MO.nearest(np.zeros((2, 3), F32), np.zeros((0, 3), F32))


# ---------------------------------------------------------------- CPU: the metrics ----------------------------------------------------------------
def test_metrics_on_concentric_spheres_and_on_one_surface_twice():
    v, f = _golden("s1_sphere")
    n = 4096
    a, b = MO.sample_surface(v, f, n, 0), MO.sample_surface(v * F32(1.05), f, n, 1)     # independent draws
    rec = MO.compare(a, b, thresholds=(0.04, 0.2))
    ra, rb = np.linalg.norm(a.points.astype(np.float64), axis=1), np.linalg.norm(b.points.astype(np.float64), axis=1)
    gap = rb.min() - ra.max()                                               # |p_b - p_a| >= |p_b| - |p_a|
    d2_ab, _ = MO.nearest(a.points, b.points)
    print(f"gap {gap:.4f} min d_ab {np.sqrt(d2_ab.min()):.4f} accuracy {rec['accuracy']:.4f} completeness {rec['completeness']:.4f}")
    assert 0.04 < gap < 0.05 and np.sqrt(d2_ab.astype(np.float64)).min() >= gap * (1 - 8 * U32)
    spacing = np.sqrt(4 * np.pi * 1.05 ** 2 / n)                            # one sample of b per spacing^2
    assert gap <= rec["accuracy"] <= np.hypot(rb.max() - ra.min(), spacing) and gap <= rec["completeness"]
    assert rec["accuracy_max"] >= rec["accuracy"] and rec["chamfer_l1"] == 0.5 * (rec["accuracy"] + rec["completeness"])
    below, above = rec["thresholds"]
    assert below["precision_count"] == below["recall_count"] == 0 and below["fscore"] == 0.0          # tau under the gap
    assert above["precision_count"] == above["recall_count"] == n and above["fscore"] == 1.0
    assert rec["dropped_ab"] == rec["dropped_ba"] == 0 and rec["normal_consistency"] > 0.99
    # one surface sampled twice: the floor is about half a sample spacing (0.028 here), and the F-score reaches 1 above it
    twice = MO.compare(a, MO.sample_surface(v, f, n, 2), thresholds=(4 * 0.028,))
    print(f"self chamfer_l1 {twice['chamfer_l1']:.4f} fscore {twice['thresholds'][0]['fscore']:.5f}")
    assert 0.02 < twice["chamfer_l1"] < 0.035 and twice["thresholds"][0]["fscore"] > 0.999
    # the same samples: zero
    same = MO.compare(a, a)
    assert same["chamfer_l1"] == 0.0 and same["chamfer_l2"] == 0.0 and same["thresholds"][0]["fscore"] == 1.0


# ---------------------------------------------------------------- CPU: plumbing and argument checks ----------------------------------------------------------------
def test_build_lists_signatures_and_defaults():
    assert {"metrics_kernels.hip", "metrics_capi.cpp"} <= set(_build.SOURCES) and "metrics.h" in _build.HEADERS
    assert _build.SOURCE_FLAGS["metrics_kernels.hip"] == ["-ffp-contract=off"]
    for name in ("metrics_kernels.hip", "metrics_capi.cpp", "metrics.h"):
        assert os.path.exists(os.path.join(_build.CSRC, name))
    assert {"tsamd_sample_surface", "tsamd_nearest_points", "tsamd_nearest_points_workspace_bytes", "tsamd_nearest_points_info"} <= set(_capi.SIGNATURES)
    assert _capi.ABI_VERSION == 3 and _capi.load().tsamd_abi_version() == 3
    from tssplat_amd import geometry, metrics
    assert inspect.signature(metrics.compare).parameters["thresholds"].default == (0.01, 0.02)
    assert inspect.signature(metrics.compare_meshes).parameters["n"].default == 100_000
    assert {"v_ref", "f_ref", "n", "seed"} <= set(inspect.signature(geometry.TetMeshGeometry.surface_metrics).parameters)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import train_object
    finally:
        sys.path.pop(0)
    assert inspect.signature(train_object.run).parameters["eval_samples"].default == 0
    assert '"--eval-samples", type=int, default=0' in inspect.getsource(train_object.main)


def test_nearest_info_reports_the_compiled_constants():
    from tssplat_amd import metrics
    info = metrics.nearest_info(100_000, 100_000)
    assert info.block % 64 == 0 and info.queries_per_lane >= 1 and info.ref_tile % 8 == 0 and info.ref_tile * 16 <= 64 * 1024
    per = info.block * info.queries_per_lane
    assert 1 <= info.auto_chunks <= -(-100_000 // info.ref_tile)
    assert metrics.nearest_info(1, 1).auto_chunks == 1 and metrics.nearest_info(0, 0).auto_chunks == 1
    assert metrics.nearest_info(1, 10 * info.ref_tile).auto_chunks == 10                      # one query block: a chunk is never less than a tile
    assert metrics.nearest_info(10_000 * per, 10 * info.ref_tile).auto_chunks == 1            # enough query blocks on their own
    lib = _capi.load()
    assert lib.tsamd_nearest_points_workspace_bytes(0) == 0 and lib.tsamd_nearest_points_workspace_bytes(5) == 40
    assert lib.tsamd_nearest_points_workspace_bytes(-1) == -1 and lib.tsamd_nearest_points_workspace_bytes(2 ** 31) == -1


def test_c_abi_argument_errors_launch_nothing():
    """Every argument error is reported before anything touches the device: all device pointers here are null or made up."""
    lib = _capi.load()
    p = 0x1000                                                              # "not null", aligned; never dereferenced on these paths
    odd, half = 0x1002, 0x1004                                              # not 4-byte, not 8-byte aligned

    def near(q=p, n=4, r=p, m=4, chunks=0, work=p, d2=p, idx=p):
        return lib.tsamd_nearest_points(q, n, r, m, chunks, work, d2, idx, None)

    def weights(v=p, nv=3, f=p, nt=1, prefix=p, work=p, phase=0):
        return lib.tsamd_sample_surface(phase, v, nv, f, nt, prefix, work, 0, 0, None, None, None, None)

    def draw(v=p, nv=3, f=p, nt=1, prefix=p, n=4, pts=p, nrm=p, tri=p):
        return lib.tsamd_sample_surface(1, v, nv, f, nt, prefix, None, n, 0, pts, nrm, tri, None)

    def info(n=4, m=4, out=(1, 1, 1, 1)):
        slots = [C.c_int32() for _ in range(4)]
        return lib.tsamd_nearest_points_info(n, m, *(C.byref(s) if keep else None for s, keep in zip(slots, out)))

    big = 2 ** 31
    cases = [
        (near, dict(n=-1), "n out"), (near, dict(n=big), "n out"), (near, dict(m=0), "m out"), (near, dict(m=-3), "m out"), (near, dict(m=big), "m out"),
        (near, dict(chunks=-1), "ref_chunks"), (near, dict(chunks=5), "ref_chunks"), (near, dict(m=70000, chunks=65536), "ref_chunks"),
        (near, dict(q=None), "query_dev"), (near, dict(r=None), "ref_dev"), (near, dict(work=None), "workspace_dev"), (near, dict(d2=None), "d2_out_dev"),
        (near, dict(idx=None), "idx_out_dev"), (near, dict(q=odd), "query_dev"), (near, dict(r=odd), "ref_dev"), (near, dict(work=half), "workspace_dev"),
        (near, dict(d2=odd), "d2_out_dev"), (near, dict(idx=odd), "idx_out_dev"),
        (weights, dict(phase=2), "phase"), (weights, dict(phase=-1), "phase"), (weights, dict(nv=-1), "n_vertices"), (weights, dict(nv=big), "n_vertices"),
        (weights, dict(nt=0), "n_triangles"), (weights, dict(nt=big), "n_triangles"), (weights, dict(v=None), "v_dev"), (weights, dict(f=None), "faces_dev"),
        (weights, dict(prefix=None), "prefix_dev"), (weights, dict(work=None), "workspace_dev"), (weights, dict(v=odd), "v_dev"),
        (weights, dict(f=odd), "faces_dev"), (weights, dict(prefix=half), "prefix_dev"), (weights, dict(work=half), "workspace_dev"),
        (draw, dict(n=-1), "n_samples"), (draw, dict(n=big), "n_samples"), (draw, dict(nt=0), "n_triangles"), (draw, dict(v=None), "v_dev"),
        (draw, dict(f=None), "faces_dev"), (draw, dict(prefix=None), "prefix_dev"), (draw, dict(pts=None), "points_out_dev"),
        (draw, dict(nrm=None), "normals_out_dev"), (draw, dict(tri=None), "tri_out_dev"), (draw, dict(prefix=half), "prefix_dev"),
        (draw, dict(pts=odd), "points_out_dev"), (draw, dict(nrm=odd), "normals_out_dev"), (draw, dict(tri=odd), "tri_out_dev"),
        (info, dict(n=-1), "n out"), (info, dict(m=big), "m out"), (info, dict(out=(0, 1, 1, 1)), "block_out"), (info, dict(out=(1, 0, 1, 1)), "queries_per_lane_out"),
        (info, dict(out=(1, 1, 0, 1)), "ref_tile_out"), (info, dict(out=(1, 1, 1, 0)), "auto_chunks_out"),
    ]
    for fn, kw, word in cases:
        assert fn(**kw) == INVALID, (fn.__name__, kw)
        msg = lib.tsamd_last_error().decode()
        assert msg and word in msg, (fn.__name__, kw, msg)
    # nothing to do is not an error, and still launches nothing: no queries, no samples
    assert near(n=0, q=None, work=None, d2=None, idx=None) == 0 and draw(n=0, pts=None, nrm=None, tri=None) == 0
    assert _capi.ABI_VERSION == 3 and lib.tsamd_abi_version() == 3          # nothing existing changed


def test_python_arguments_are_checked_by_name():
    """Nothing here reaches the library: a CPU tensor, a wrong dtype or shape is refused first, with the argument's name."""
    from tssplat_amd import metrics
    v, f, pts = torch.zeros(4, 3), torch.zeros(1, 3, dtype=torch.int32), torch.zeros(5, 3)
    s = metrics.SurfaceSamples(pts, pts, torch.zeros(5, dtype=torch.int32))
    for call, word in [(lambda: metrics.sample_surface(v, f, 4), "v must be a GPU tensor"), (lambda: metrics.sample_surface(np.zeros((4, 3), F32), f, 4), "v must"),
                       (lambda: metrics.nearest(pts, pts), "query must"), (lambda: metrics.nearest(None, pts), "query must"),
                       (lambda: metrics.compare(s, s), r"a\.points must"), (lambda: metrics.compare(pts, s), "a must be SurfaceSamples"),
                       (lambda: metrics.compare_meshes(v, f, v, f, n=0), "n must be"), (lambda: metrics.compare_meshes(v, f, v, f, n=10), "v_a must"),
                       (lambda: metrics.compare_meshes(v, f, v, f, thresholds=(-1.0,)), "thresholds must"),
                       (lambda: metrics.compare_meshes(v, f, v, f, seed=0.5), "seed must"), (lambda: metrics.nearest_info(-1, 4), "n must be")]:
        with pytest.raises(RuntimeError, match=word):
            call()
    with pytest.raises(RuntimeError, match="n must be"):
        metrics._check_count("sample_surface", "n", 2 ** 31)
    assert metrics._check_seed("sample_surface", -1) == 2 ** 64 - 1


@gpu
def test_python_arguments_on_the_device_are_checked_by_name():
    from tssplat_amd import metrics
    v, f = (dev(x) for x in _one_triangle())
    pts = dev(np.zeros((5, 3), F32))
    for call, word in [(lambda: metrics.sample_surface(v.double(), f, 4), "v must be float32"), (lambda: metrics.sample_surface(v, f.long(), 4), "faces must be int32"),
                       (lambda: metrics.sample_surface(v[:, :2], f, 4), r"v must be \[N, 3\]"), (lambda: metrics.sample_surface(v, f[:, :2], 4), r"faces must be \[N, 3\]"),
                       (lambda: metrics.sample_surface(v.T.contiguous().T, f, 4), "v must be contiguous"), (lambda: metrics.sample_surface(v, f, -1), "n must be"),
                       (lambda: metrics.sample_surface(v, f, 4, seed="x"), "seed must"), (lambda: metrics.sample_surface(v, f[:0], 4), "faces holds no triangle"),
                       (lambda: metrics.sample_surface(v, f * 0, 4), "faces holds no triangle of positive area"),
                       (lambda: metrics.sample_surface(v[:0], f, 4), "faces holds no triangle of positive area"),
                       (lambda: metrics.nearest(pts, pts[:0]), "ref holds no point"), (lambda: metrics.nearest(pts, pts.cpu()), "ref must be a GPU"),
                       (lambda: metrics.nearest(pts, pts, ref_chunks=6), "ref_chunks must"), (lambda: metrics.nearest(pts, pts, ref_chunks=-1), "ref_chunks must"),
                       (lambda: metrics.nearest(pts.reshape(-1), pts), r"query must be \[N, 3\]"),
                       (lambda: metrics.compare(metrics.SurfaceSamples(pts, pts[:4], None), metrics.SurfaceSamples(pts, pts, None)), r"a\.normals must have"),
                       (lambda: metrics.compare(metrics.SurfaceSamples(pts[:0], pts[:0], None), metrics.SurfaceSamples(pts, pts, None)), r"a\.points holds no sample")]:
        with pytest.raises(RuntimeError, match=word):
            call()
    d2, idx = metrics.nearest(pts[:0], pts)                                  # N == 0: empty tensors
    assert tuple(d2.shape) == (0,) and d2.dtype == torch.float32 and tuple(idx.shape) == (0,) and idx.dtype == torch.int32
    s = metrics.sample_surface(v, f, 0)                                      # n == 0: empty tensors
    assert tuple(s.points.shape) == (0, 3) and tuple(s.normals.shape) == (0, 3) and tuple(s.tri.shape) == (0,)


# ---------------------------------------------------------------- GPU: nearest ----------------------------------------------------------------
def _nearest_both(q, r, **kw):
    from tssplat_amd import metrics
    want_d2, want_idx = MO.nearest(q, r)
    d2, idx = metrics.nearest(dev(q), dev(r), **kw)
    assert d2.dtype == torch.float32 and idx.dtype == torch.int32
    d2, idx = d2.cpu().numpy(), idx.cpu().numpy()
    assert idx.tobytes() == want_idx.tobytes(), (kw, int((idx != want_idx).sum()))
    assert d2.tobytes() == want_d2.tobytes(), (kw, int((d2.view(np.uint32) != want_d2.view(np.uint32)).sum()))
    return want_d2, want_idx


def _info():
    from tssplat_amd import metrics
    return metrics.nearest_info(1, 1)


def _cloud(n, seed):
    """Points on a coarse grid of 1/8 steps, so that equal distances and repeated points occur, in float32."""
    return (np.random.default_rng(seed).integers(-24, 25, (n, 3)) / 8.0).astype(F32)


@gpu
@pytest.mark.parametrize("which", ["1", "63", "64", "65", "per-1", "per+1"])
def test_nearest_sizes_equal_oracle(which):
    info = _info()
    per, tile = info.block * info.queries_per_lane, info.ref_tile
    N = {"1": 1, "63": 63, "64": 64, "65": 65, "per-1": per - 1, "per+1": per + 1}[which]
    for M in (1, 2, tile - 1, tile, tile + 1, 2 * tile + 3):
        _nearest_both(_cloud(N, 100 + N), _cloud(M, 200 + M))
        _nearest_both(np.random.default_rng(N + M).standard_normal((N, 3)).astype(F32), np.random.default_rng(N * M).standard_normal((M, 3)).astype(F32))


@gpu
def test_nearest_does_not_depend_on_the_chunk_count():
    info = _info()
    M = 2 * info.ref_tile + 3
    q, r = _cloud(65, 1), np.random.default_rng(2).standard_normal((M, 3)).astype(F32)
    r[M - 2] = r[5] = q[0]                                                   # an exact tie between the first and the last chunk: row 5 wins
    r[M - 1] = r[M // 2 + 1] = q[1]                                          # and between the middle and the end
    for chunks in (0, 1, 2, 7, M):
        _, idx = _nearest_both(q, r, ref_chunks=chunks)
        assert idx[0] == 5 and idx[1] == M // 2 + 1
    big = np.random.default_rng(3).standard_normal((3 * info.block * info.queries_per_lane + 17, 3)).astype(F32)
    for chunks in (0, 3):
        _nearest_both(big, r, ref_chunks=chunks)                             # several query blocks times several chunks


@gpu
def test_nearest_ties_go_to_the_lowest_index():
    lattice = np.stack(np.meshgrid(*[np.arange(5)] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(F32)
    centres = (np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), axis=-1).reshape(-1, 3) + 0.5).astype(F32)
    faces = centres.copy()
    faces[:, 2] -= 0.5
    for q, value in ((centres, 0.75), (faces, 0.5)):                         # 8 and 4 exactly tied minima (checked on the CPU above)
        for ref in (lattice, np.concatenate([lattice, lattice]), np.concatenate([lattice[::-1], lattice])):
            for chunks in (0, 1, 5, ref.shape[0]):
                d2, idx = _nearest_both(q, ref, ref_chunks=chunks)
                assert (d2 == value).all()
    d2, idx = _nearest_both(centres, np.concatenate([lattice, lattice]))
    assert idx.max() < 125


@gpu
def test_nearest_special_values():
    nan, inf = np.nan, np.inf
    rng = np.random.default_rng(5)
    q, r = rng.standard_normal((70, 3)).astype(F32), rng.standard_normal((1500, 3)).astype(F32)
    q[3], q[10], q[20], q[30, 1], q[40, 2] = nan, inf, -inf, nan, -inf
    r[0], r[7], r[100], r[1100, 0], r[1200, 1], r[1499] = nan, inf, -inf, nan, inf, nan
    for chunks in (0, 1, 2, 1500):
        d2, idx = _nearest_both(q, r, ref_chunks=chunks)
    assert idx[3] == -1 and d2[3] == inf and idx[30] == -1                   # a NaN coordinate: every pair is a NaN
    assert d2[10] == inf and idx[10] == 1                                    # an all-inf query: inf - inf is a NaN at row 7, +inf is an ordinary value at row 1
    d2, idx = _nearest_both(q, np.full((9, 3), nan, F32))                    # an all-NaN ref
    assert (idx == -1).all() and (d2 == inf).all()
    far = (rng.uniform(-2e19, 2e19, (200, 3))).astype(F32)                   # squares and sums overflow to +inf
    d2, idx = _nearest_both(far[:60], far[60:])
    assert np.isfinite(d2).any() and (idx >= 0).all()
    d2, idx = _nearest_both(np.full((2, 3), 3e38, F32), np.full((4, 3), -3e38, F32))
    assert (d2 == inf).all() and (idx == 0).all()                            # every pair +inf: the lowest index, not -1


# ---------------------------------------------------------------- GPU: the sampler ----------------------------------------------------------------
def _sample_both(mesh, n, seed):
    from tssplat_amd import metrics
    v, f = MESHES[mesh]()
    want = _oracle_samples(mesh, 1000, seed)                                # counter-based: the first n samples of any longer run
    got = metrics.sample_surface(dev(v), dev(f), n, seed)
    assert got.points.dtype == got.normals.dtype == torch.float32 and got.tri.dtype == torch.int32
    assert tuple(got.points.shape) == tuple(got.normals.shape) == (n, 3) and tuple(got.tri.shape) == (n,)
    tri, pts, nrm = got.tri.cpu().numpy(), got.points.cpu().numpy(), got.normals.cpu().numpy()
    assert tri.tobytes() == want.tri[:n].tobytes(), int((tri != want.tri[:n]).sum())
    assert pts.tobytes() == want.points[:n].tobytes(), int((pts.view(np.uint32) != want.points[:n].view(np.uint32)).sum())
    assert nrm.tobytes() == want.normals[:n].tobytes(), int((nrm.view(np.uint32) != want.normals[:n].view(np.uint32)).sum())
    return tri


@gpu
@pytest.mark.parametrize("mesh", sorted(MESHES))
def test_sampler_equals_oracle(mesh):
    for n in (1, 63, 64, 65, 1000):
        tri = _sample_both(mesh, n, seed=0)
    _sample_both(mesh, 1000, seed=2 ** 64 - 1)
    if mesh == "hostile":
        assert set(np.unique(tri).tolist()) == set(DRAWABLE)


@gpu
def test_sampler_is_repeatable_and_seeds_differ():
    from tssplat_amd import metrics
    v, f = (dev(x) for x in _golden("mario_mesh"))
    a, b, c = metrics.sample_surface(v, f, 5000, 4), metrics.sample_surface(v, f, 5000, 4), metrics.sample_surface(v, f, 5000, 5)
    for x, y in ((a.points, b.points), (a.normals, b.normals), (a.tri, b.tri)):
        assert torch.equal(x, y)
    assert float((a.tri == c.tri).float().mean()) < 0.01 and not torch.equal(a.points, c.points)
    assert torch.equal(metrics.sample_surface(v, f, 100, 4).points, a.points[:100])


# ---------------------------------------------------------------- GPU: compare ----------------------------------------------------------------
FLOAT_FIELDS = ("chamfer_l1", "chamfer_l2", "accuracy", "completeness", "accuracy_max", "completeness_max", "normal_consistency")


def _assert_record_close(got, want, n):
    """Integers equal; floats within the rounding of a float64 mean of n float32 square roots.  d2 and idx are the oracle's bits, so
    only the square root (the device's within one ulp, 2 U of d; numpy's correctly rounded, U), and the order of the float64 sums
    (n U64 relative on sums of non-negative terms, each side) differ: |mean - mean'| <= (3 U32 + 2 n U64) mean.  chamfer_l2 has no root,
    the cosines are three exact products and two sums (2 U64) before theirs."""
    g = got.as_dict()
    for key in ("n_a", "n_b", "dropped_ab", "dropped_ba"):
        assert g[key] == want[key], key
    for tg, tw in zip(g["thresholds"], want["thresholds"]):
        assert (tg["precision_count"], tg["recall_count"], tg["tau"]) == (tw["precision_count"], tw["recall_count"], tw["tau"])
        for key in ("precision", "recall", "fscore"):
            assert tg[key] == tw[key], key                                   # the same integers through the same float64 operations
    rel = {"chamfer_l2": 2 * n * U64, "normal_consistency": (2 * n + 4) * U64}
    for key in FLOAT_FIELDS:
        bound = rel.get(key, 3 * U32 + 2 * n * U64) * abs(want[key])
        print(f"{key}: {g[key]!r} oracle {want[key]!r} |diff| {abs(g[key] - want[key]):.3e} bound {bound:.3e}")
        assert abs(g[key] - want[key]) <= bound, key


@gpu
def test_compare_equals_oracle_and_is_bitwise_repeatable():
    from tssplat_amd import metrics
    v, f = _golden("s1_sphere")
    n = 3000
    sa, sb = _oracle_samples("s1_sphere", 1000, 0), MO.sample_surface(v * F32(1.05), f, n, 9)
    a = metrics.SurfaceSamples(dev(sa.points), dev(sa.normals), dev(sa.tri))                  # N != M
    b = metrics.SurfaceSamples(dev(sb.points), dev(sb.normals), dev(sb.tri))
    taus = (0.05, 0.06, 0.2)
    got, again = metrics.compare(a, b, thresholds=taus), metrics.compare(a, b, thresholds=taus)
    assert got.as_dict() == again.as_dict() and repr(got) == repr(again)                      # bit for bit
    _assert_record_close(got, MO.compare(sa, sb, thresholds=taus), n)
    assert got.noise_floor is None and 0 < got.thresholds[1].precision_count < 1000          # a threshold that cuts through the samples
    # dropped samples: a NaN point has no nearest point, and nobody's nearest point is it
    pts = sa.points.copy()
    pts[[5, 17]] = np.nan
    holed = metrics.SurfaceSamples(dev(pts), a.normals, a.tri)
    got = metrics.compare(holed, b, thresholds=taus)
    assert got.dropped_ab == 2 and got.dropped_ba == 0
    _assert_record_close(got, MO.compare(SimpleNamespace(points=pts, normals=sa.normals), sb, thresholds=taus), n)


@gpu
def test_compare_meshes_against_its_noise_floor():
    """One mesh against itself: `a` (seed + 2), `b` (seed) and the floor's second sampling (seed + 1) are three independent samplings of one
    surface, so chamfer_l1 and noise_floor estimate the same number.  Each is a mean over 2 n nearest distances whose coefficient of
    variation is that of a Rayleigh variable, 0.52: their ratio has a standard deviation of 0.52 sqrt(2 / 2n) = 0.8 % at n = 4096, and the
    stated factor 1.1 is twelve of them.  Measured: chamfer_l1 0.016970, noise_floor 0.016986, ratio 0.9991, each equal to the oracle's
    value for the same seeds in every bit."""
    from tssplat_amd import metrics
    v, f = _golden("mario_mesh")
    n, seed = 4096, 0
    got = metrics.compare_meshes(dev(v), dev(f), dev(v), dev(f), n=n, seed=seed)
    sb = MO.sample_surface(v, f, n, seed)
    want = MO.compare(MO.sample_surface(v, f, n, seed + 2), sb)
    floor = MO.compare(sb, MO.sample_surface(v, f, n, seed + 1))["chamfer_l1"]
    _assert_record_close(got, want, n)
    print(f"chamfer_l1 {got.chamfer_l1!r} noise_floor {got.noise_floor!r} oracle {want['chamfer_l1']!r} {floor!r} ratio {got.chamfer_l1 / got.noise_floor:.4f}")
    assert abs(got.noise_floor - floor) <= (3 * U32 + 2 * n * U64) * floor
    assert got.noise_floor / 1.1 < got.chamfer_l1 < 1.1 * got.noise_floor
    # a copy scaled by 1.1 moves the surface by a tenth of |p| along p; at the default 100 000 samples the floor is half a sample
    # spacing, a few thousandths of the unit ball the mesh fills: clearly apart
    scaled = metrics.compare_meshes(dev(v * F32(1.1)), dev(f), dev(v), dev(f))
    print(f"scaled by 1.1: chamfer_l1 {scaled.chamfer_l1:.5f} noise_floor {scaled.noise_floor:.5f} fscore@0.01 {scaled.thresholds[0].fscore:.4f}")
    assert scaled.n_a == scaled.n_b == 100_000 and scaled.chamfer_l1 > 3 * scaled.noise_floor
    same = metrics.compare_meshes(dev(v), dev(f), dev(v), dev(f))
    assert same.noise_floor == scaled.noise_floor and same.thresholds[0].fscore > scaled.thresholds[0].fscore


@gpu
def test_geometry_surface_metrics_is_compare_meshes_of_its_boundary():
    from tssplat_amd import geometry, metrics, scenes
    bv, bt = scenes.kuhn_ball(4)
    bv = (bv / np.linalg.norm(bv, axis=1).max()).astype(F32)
    geo = geometry.TetMeshGeometry(bv, bt.astype(np.int32), use_smooth_barrier=False)
    v, f = (dev(x) for x in _golden("s1_sphere"))
    got = geo.surface_metrics(v, f, n=2000, seed=3)
    want = metrics.compare_meshes(geo.tet_v.detach()[geo.surface_vid.long()].contiguous(), geo.surface_fid, v, f, n=2000, seed=3)
    assert got.as_dict() == want.as_dict() and got.noise_floor > 0 and got.chamfer_l1 < 0.2


# ---------------------------------------------------------------- edges: exact ties in the sampler ----------------------------------------------------------------
# Random float data meets an equal pair of operands only by accident: through sample_surface the total weight Q is about T 2^32, so
# p == C[t] has probability T / 2^32 per sample, and ia + ib == 2^24 has 2^-24.  Here the prefix sums are written by hand and handed to
# the draw phase of the C ABI, the seeds are chosen so that sample 0 sits on the fold, and the weights phase is compared on its own.
def _lattice_mesh(T):
    """T isolated right triangles with unit legs on the integer lattice of the plane z = 0: equal areas, every coordinate exact."""
    t = np.arange(T)
    v = np.zeros((T, 3, 3), F32)
    v[:, :, 0] = (2 * (t % 16))[:, None]
    v[:, :, 1] = (2 * (t // 16))[:, None]
    v[:, 1, 0] += 1
    v[:, 2, 1] += 1
    return v.reshape(-1, 3), np.arange(3 * T, dtype=np.int32).reshape(T, 3)


def _tiny_weight_mesh():
    """Right triangles with legs 2^10, 2^-7, 2^-6: w = 2^20, 2^-14, 2^-12, so w / w_max = 1, 2^-34, 2^-32 and q = 2^32, 0, 1 -- the
    second one has a positive area and is never drawn, the third one is the smallest weight that is."""
    legs = [2.0 ** 10, 2.0 ** -7, 2.0 ** -6]
    v = np.array([[[0, 0, 0], [s, 0, 0], [0, s, 0]] for s in legs], F32).reshape(-1, 3)
    return v, np.arange(9, dtype=np.int32).reshape(3, 3)


PREFIXES = {"one": [1], "three": [1, 2, 3], "zeros": [0, 0, 1, 1, 2, 3, 3],                      # zero weights leading, in a run, trailing
            "equal255": [2 * (t + 1) for t in range(255)], "equal256": [2 * (t + 1) for t in range(256)], "equal257": [2 * (t + 1) for t in range(257)],
            "huge": [2 ** 60, 2 ** 60, 3 * 2 ** 60, 2 ** 62, 2 ** 62]}
DRAW_N, DRAW_SEED = 4096, 0


@functools.lru_cache(maxsize=None)
def _oracle_draw(name):
    return MO.draw(*_lattice_mesh(len(PREFIXES[name])), PREFIXES[name], DRAW_N, DRAW_SEED)


@pytest.mark.parametrize("name", sorted(PREFIXES))
def test_edge_hand_made_prefixes_are_reached(name):
    """From the oracle and the prefix alone: every p in [0, Q) occurs where Q is small, so p == C[t - 1] (the first value that belongs to
    t: `>=` for `>` in the search sends it to t - 1) and p == C[t] - 1 (the last) occur for every drawable t; no triangle of weight 0 is
    drawn; and the triangle is the first with C[t] > p by Python's own bisection."""
    import bisect
    prefix = PREFIXES[name]
    weight = np.diff([0] + prefix).tolist()
    assert min(weight) >= 0 and prefix[-1] > 0                               # a genuine prefix
    area = MO.face_normals(*_lattice_mesh(len(prefix)))[1]
    assert (area == 1.0).all()                                               # valid triangles of positive area, zero weight or not
    s = _oracle_draw(name)
    drawable = [t for t, w in enumerate(weight) if w > 0]
    p = [int(x) for x in s.p]
    assert s.Q == prefix[-1] and 0 <= min(p) and max(p) < s.Q
    assert s.tri.tolist() == [bisect.bisect_right(prefix, x) for x in p]
    assert sorted(set(s.tri.tolist())) == drawable
    first = sum(1 for t in drawable if prefix[t] - weight[t] in set(p))
    last = sum(1 for t in drawable if prefix[t] - 1 in set(p))
    print(f"{name}: Q {s.Q} distinct p {len(set(p))} drawable {len(drawable)} with p == C[t-1] {first} with p == C[t]-1 {last}")
    if s.Q < 1024:
        assert set(p) == set(range(s.Q)) and first == last == len(drawable)
    else:
        assert s.Q == 2 ** 62 and len(set(p)) == DRAW_N                      # 64-bit products: the high word of u Q, not a 32-bit shortcut
    assert MO.draw(*_lattice_mesh(len(prefix)), prefix, 5, DRAW_SEED).tri.tolist() == s.tri[:5].tolist()
    assert MO.draw(*_lattice_mesh(len(prefix)), prefix, 0, DRAW_SEED).points.shape == (0, 3)


def test_edge_draw_is_the_tail_of_sample_surface():
    """sample_surface is integer_weights, a prefix sum and draw: the same samples from the prefix handed over by hand."""
    v, f = _golden("s1_sphere")
    s = _oracle_samples("s1_sphere", 1000, 0)
    d = MO.draw(v, f, np.cumsum([int(x) for x in MO.integer_weights(v, f)], dtype=object), 1000, 0)
    for key in ("tri", "points", "normals", "a", "b"):
        assert getattr(d, key).tobytes() == getattr(s, key).tobytes(), key
    assert d.Q == s.Q and s.q.tolist() == MO.integer_weights(v, f).tolist()


# sample i of seed 0 is sample 0 of seed 3 i GOLDEN mod 2^64: found by scanning i < 2^26 with mix64_array
FOLD_SEEDS = {"sum == 2^24": 0x6F0B2F4A11BFEDF0, "sum == 2^24 + 1": 0xE1B751B607FDBFC7, "sum == 2^24 - 1": 0x1413E1F979F588EE, "ia == 0": 0xFD2DD52195A0B661,
              "ib == 0": 0x931E3C944A5C6B0D}


def _first_barycentrics(seed):
    return MO.mix64(seed, 1) >> 40, MO.mix64(seed, 2) >> 40


def test_edge_fold_seeds_are_reached():
    one = 1 << 24
    got = {name: _first_barycentrics(seed) for name, seed in FOLD_SEEDS.items()}
    print(got)
    assert got["sum == 2^24"] == (16032853, 744363) and sum(got["sum == 2^24"]) == one
    assert sum(got["sum == 2^24 + 1"]) == one + 1 and sum(got["sum == 2^24 - 1"]) == one - 1
    assert got["ia == 0"][0] == 0 and got["ib == 0"][1] == 0
    v, f = _one_triangle()
    for name, seed in FOLD_SEEDS.items():
        s = MO.sample_surface(v, f, 1, seed)
        ia, ib = got[name]
        folded = ia + ib > one
        assert folded == (name == "sum == 2^24 + 1")                         # a + b == 1 stays: the point lies on the edge B C
        want = (one - ia, one - ib) if folded else (ia, ib)
        assert (float(s.a[0]) * one, float(s.b[0]) * one) == want


def test_edge_weights_are_reached():
    for T in (255, 256, 257):
        assert MO.integer_weights(*_lattice_mesh(T)).tolist() == [2 ** 32] * T
    v, f = _tiny_weight_mesh()
    assert MO.face_normals(v, f)[1].tolist() == [2.0 ** 20, 2.0 ** -14, 2.0 ** -12] and MO.integer_weights(v, f).tolist() == [2 ** 32, 0, 1]
    assert set(MO.sample_surface(v, f, 4096, 0).tri.tolist()) == {0}         # weight 1 in 2^32 + 1: not in 4096 draws; weight 0: never


def _draw_on_device(v, f, prefix, n, seed):
    """Phase DRAW of tsamd_sample_surface with the caller's own prefix sums."""
    from tssplat_amd import _args
    vd, fd, cd = dev(v), dev(f), dev(np.asarray(prefix, dtype=np.int64))
    lib, ctx, stream = _args.lib_and_stream(vd.device)
    pts, nrm = torch.empty((n, 3), dtype=torch.float32, device=vd.device), torch.empty((n, 3), dtype=torch.float32, device=vd.device)
    tri = torch.empty(n, dtype=torch.int32, device=vd.device)
    with ctx:
        _capi.check(lib.tsamd_sample_surface(1, vd.data_ptr(), v.shape[0], fd.data_ptr(), f.shape[0], cd.data_ptr(), None, n, seed, pts.data_ptr(), nrm.data_ptr(),
                                             tri.data_ptr(), stream))
    return tri.cpu().numpy(), pts.cpu().numpy(), nrm.cpu().numpy()


def _weights_on_device(v, f):
    """Phase WEIGHTS of tsamd_sample_surface: the int64 q, before any prefix sum."""
    from tssplat_amd import _args
    vd, fd = dev(v), dev(f)
    lib, ctx, stream = _args.lib_and_stream(fd.device)
    q = torch.full((f.shape[0],), -1, dtype=torch.int64, device=fd.device)
    work = torch.empty(1, dtype=torch.int64, device=fd.device)
    with ctx:
        _capi.check(lib.tsamd_sample_surface(0, _args.ptr(vd), v.shape[0], fd.data_ptr(), f.shape[0], q.data_ptr(), work.data_ptr(), 0, 0, None, None, None, stream))
    return q.cpu().numpy()


@gpu
@pytest.mark.parametrize("name", sorted(PREFIXES))
def test_edge_hand_made_prefixes(name):
    prefix = PREFIXES[name]
    v, f = _lattice_mesh(len(prefix))
    want = _oracle_draw(name)
    tri, pts, nrm = _draw_on_device(v, f, prefix, DRAW_N, DRAW_SEED)
    assert tri.tobytes() == want.tri.tobytes(), (int((tri != want.tri).sum()), tri[tri != want.tri][:8], want.tri[tri != want.tri][:8])
    assert pts.tobytes() == want.points.tobytes() and nrm.tobytes() == want.normals.tobytes()


@gpu
@pytest.mark.parametrize("name", sorted(FOLD_SEEDS))
def test_edge_fold_seeds(name):
    seed = FOLD_SEEDS[name]
    for mesh in ("one_triangle", "s1_sphere"):
        _sample_both(mesh, 64, seed)
    if name == "sum == 2^24":                                                # sample 0 keeps its barycentrics: folded, they would be exchanged
        from tssplat_amd import metrics
        v, f = _one_triangle()
        ia, ib = _first_barycentrics(seed)
        A, B, Cc = v[0], v[1], v[2]

        def point(x, y):
            return (A + F32(x * 2.0 ** -24) * (B - A)) + F32(y * 2.0 ** -24) * (Cc - A)
        assert point(ia, ib).tobytes() != point(ib, ia).tobytes()
        got = metrics.sample_surface(dev(v), dev(f), 1, seed).points.cpu().numpy()[0]
        assert got.tobytes() == point(ia, ib).tobytes()


@gpu
def test_edge_weights_phase_equals_integer_weights():
    cases = [(name, make()) for name, make in sorted(MESHES.items())] + [(f"lattice{T}", _lattice_mesh(T)) for T in (255, 256, 257)]
    cases.append(("tiny", _tiny_weight_mesh()))
    for name, (v, f) in cases:
        want = MO.integer_weights(v, f)
        got = _weights_on_device(v, f)
        assert got.dtype == np.int64 and got.astype(np.uint64).tobytes() == want.tobytes(), (name, int((got.astype(np.uint64) != want).sum()))
    assert got.tolist() == [2 ** 32, 0, 1]                                   # the last case: a positive area that is never drawn
