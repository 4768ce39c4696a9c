"""The argument errors of the surface stages (spheres_init, merge, metrics, simplify, voxelize and their C entry points), pinned to the
byte: a table of calls and the exact text each one raises or leaves in ``tsamd_last_error()``, compared with ``==``.  A row with two
things wrong at once pins the order of the checks.  Nothing here launches a kernel: device pointers are null or made up, and the
``gpu`` rows only need tensors that live on a device to get past a module's first check."""
import ctypes as C

import numpy as np
import pytest
import torch

from tssplat_amd import _capi, merge, metrics, simplify, spheres_init, voxelize

gpu = pytest.mark.gpu
INVALID = 1     # TSAMD_ERR_INVALID_ARGUMENT
nan, inf = float("nan"), float("inf")
UNIT = (-1.0, 1.0)
OVERFLOW = (-1e308, 1e308)      # finite ends, hi - lo = inf

GPU = " must be a GPU tensor (there is no CPU fallback)"
BOUNDS = "bounds must be (lo, hi), finite, with lo < hi, got "
BAD_BOUNDS = [(3, "3"), ((0.0, 1.0, 2.0), "(0.0, 1.0, 2.0)"), ((1.0, -1.0), "(1.0, -1.0)"), ((1.0, 1.0), "(1.0, 1.0)"), ((nan, 1.0), "(nan, 1.0)"),
              ((0.0, inf), "(0.0, inf)")]
OVERFLOW_TEXT = "(-1e+308, 1e+308)"
TINY = ((0.0, 5e-324), "(0.0, 5e-324)")      # (hi - lo) / cells underflows to 0: simplify and voxelize only


def bounds_rows(fn, cases):
    return [(lambda b=b: fn(b), BOUNDS + text) for b, text in cases]


def mismatches(tables):
    """[(prefix + row number, got, want)] over ``[(prefix, [(call, want), ...]), ...]``; every call must raise RuntimeError."""
    bad = []
    for prefix, rows in tables:
        for k, (call, want) in enumerate(rows):
            try:
                call()
                got = "<no error>"
            except RuntimeError as err:
                got = str(err)
            if got != prefix + want:
                bad.append((f"{prefix}#{k}", got, prefix + want))
    return bad


# ---------------------------------------------------------------- Python, without a device ----------------------------------------------------------------
v, f, e = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(1, 4, dtype=torch.int32)
fld, pts = torch.zeros(4, 4, 4), torch.zeros(5, 3)
alpha, mvp = torch.zeros(1, 8, 8, 1), torch.zeros(1, 4, 4)
occ = torch.zeros(4, 4, 4, dtype=torch.bool)
vn = np.zeros((4, 3), np.float32)
samples = metrics.SurfaceSamples(pts, pts, torch.zeros(5, dtype=torch.int32))

SI, MG, MT, SP, VX = ("tssplat_amd.%s." % m for m in ("spheres_init", "merge", "metrics", "simplify", "voxelize"))
G512 = "grid must be an integer in 1 .. 512, got "
G2 = "grid must be an integer in 2 .. 512, got "
CELLS = "cells must be an integer in 1 .. 1024, got "
NSPH = "n_spheres must be an integer in 0 .. 2^20, got "
COUNT0 = " must be an integer in 0 .. 2^31 - 1, got "
ROWS_V = "v must be [N, 3] with N <= 2147483647, got "
ROWS_F = "faces must be [N, 3] with N <= 715827882, got "
FILL = "fill must be one of 'none', 'cavities', 'outer', got "
RULE = "rule must be one of 'nonzero', 'positive', 'odd', got "

CPU_TABLES = [
    # ---- spheres_init: grid, bounds, then the tensors (the device before dtype and shape) ----
    (SI + "voxel_centres: ", [
        (lambda: spheres_init.voxel_centres(0), G512 + "0"), (lambda: spheres_init.voxel_centres(513), G512 + "513"),
        (lambda: spheres_init.voxel_centres(True), G512 + "True"), (lambda: spheres_init.voxel_centres(2.0), G512 + "2.0"),
        (lambda: spheres_init.voxel_centres(0, (1.0, 1.0)), G512 + "0"),
    ] + bounds_rows(lambda b: spheres_init.voxel_centres(4, b), BAD_BOUNDS + [(None, "None")])),
    (SI + "visual_hull: ", [
        (lambda: spheres_init.visual_hull(alpha, mvp), "alpha" + GPU), (lambda: spheres_init.visual_hull(None, mvp), "alpha" + GPU),
        (lambda: spheres_init.visual_hull(alpha.numpy(), mvp), "alpha" + GPU), (lambda: spheres_init.visual_hull(alpha.double(), mvp), "alpha" + GPU),
        (lambda: spheres_init.visual_hull(alpha, mvp, grid=0), G512 + "0"), (lambda: spheres_init.visual_hull(alpha, mvp, grid=513), G512 + "513"),
        (lambda: spheres_init.visual_hull(alpha, mvp, grid=1), "alpha" + GPU), (lambda: spheres_init.visual_hull(alpha, mvp, grid=512), "alpha" + GPU),
        (lambda: spheres_init.visual_hull(alpha, mvp, grid=0, bounds=(1.0, 1.0)), G512 + "0"),
        (lambda: spheres_init.visual_hull(None, mvp, channel=-1, threshold=nan), "alpha" + GPU),
    ] + bounds_rows(lambda b: spheres_init.visual_hull(None, mvp, bounds=b), BAD_BOUNDS)),
    (SI + "distance_transform_sq: ", [
        (lambda: spheres_init.distance_transform_sq(occ), "mask" + GPU), (lambda: spheres_init.distance_transform_sq(None), "mask" + GPU),
        (lambda: spheres_init.distance_transform_sq(fld[:2]), "mask" + GPU),
    ]),
    (SI + "greedy_cover: ", [
        (lambda: spheres_init.greedy_cover(occ, occ.int(), 1), "hull" + GPU), (lambda: spheres_init.greedy_cover(None, None, -1, bounds=3), "hull" + GPU),
    ]),
    (SI + "init_spheres: ", [
        (lambda: spheres_init.init_spheres(alpha, mvp, -1), NSPH + "-1"), (lambda: spheres_init.init_spheres(alpha, mvp, (1 << 20) + 1), NSPH + "1048577"),
        (lambda: spheres_init.init_spheres(alpha, mvp, True), NSPH + "True"), (lambda: spheres_init.init_spheres(alpha, mvp, 2.0), NSPH + "2.0"),
        (lambda: spheres_init.init_spheres(alpha, mvp, 0, min_radius=-1.0), "min_radius must be finite and not negative, got -1.0"),
        (lambda: spheres_init.init_spheres(alpha, mvp, 1 << 20, min_radius=nan), "min_radius must be finite and not negative, got nan"),
        (lambda: spheres_init.init_spheres(alpha, mvp, 2, min_radius=inf, shrink=0.0), "min_radius must be finite and not negative, got inf"),
        (lambda: spheres_init.init_spheres(alpha, mvp, 2, shrink=0.0), "shrink must be finite and positive, got 0.0"),
        (lambda: spheres_init.init_spheres(alpha, mvp, 2, shrink=nan), "shrink must be finite and positive, got nan"),
        (lambda: spheres_init.init_spheres(alpha, mvp, -1, grid=0), NSPH + "-1"), (lambda: spheres_init.init_spheres(alpha, mvp, 2, grid=0), G512 + "0"),
        (lambda: spheres_init.init_spheres(alpha, mvp, 2), "alpha" + GPU),
    ] + bounds_rows(lambda b: spheres_init.init_spheres(alpha, mvp, 2, bounds=b), BAD_BOUNDS)),
    (SI + "cover_occupancy: ", [
        (lambda: spheres_init.cover_occupancy(occ, 3), "occ" + GPU), (lambda: spheres_init.cover_occupancy(vn, -1, bounds=3), "occ" + GPU),
    ]),
    # ---- merge: the tensors first (the device before dtype and shape), then grid, bounds, level ----
    (MG + "default_level: ", [
        (lambda: merge.default_level(1, UNIT), G2 + "1"), (lambda: merge.default_level(513, UNIT), G2 + "513"), (lambda: merge.default_level(True, UNIT), G2 + "True"),
        (lambda: merge.default_level(8.0, UNIT), G2 + "8.0"), (lambda: merge.default_level(1, (1.0, 1.0)), G2 + "1"),
    ] + bounds_rows(lambda b: merge.default_level(8, b), BAD_BOUNDS + [(OVERFLOW, OVERFLOW_TEXT), (None, "None")])),
    (MG + "default_bounds: ", [
        (lambda: merge.default_bounds(v, 4), "grid must be an integer in 5 .. 512, got 4"), (lambda: merge.default_bounds(v, 513), "grid must be an integer in 5 .. 512, got 513"),
        (lambda: merge.default_bounds(v, 5), "tet_v" + GPU), (lambda: merge.default_bounds(v, 512), "tet_v" + GPU), (lambda: merge.default_bounds(vn, 8), "tet_v" + GPU),
    ]),
    (MG + "union_field: ", [
        (lambda: merge.union_field(v, e, 8, UNIT), "tet_v" + GPU), (lambda: merge.union_field(None, e, 8, UNIT), "tet_v" + GPU),
        (lambda: merge.union_field(vn, e, 8, UNIT), "tet_v" + GPU), (lambda: merge.union_field(v.double(), e, 8, UNIT), "tet_v" + GPU),
        (lambda: merge.union_field(v[:, :2], e.long(), 1, (1.0, 1.0)), "tet_v" + GPU),
    ]),
    (MG + "extract_surface: ", [(lambda: merge.extract_surface(fld, UNIT, 0.0), "field" + GPU), (lambda: merge.extract_surface(None, 3, nan), "field" + GPU)]),
    (MG + "occupancy: ", [(lambda: merge.occupancy(fld, 0.0), "field" + GPU), (lambda: merge.occupancy(fld.double(), nan), "field" + GPU)]),
    (MG + "components: ", [(lambda: merge.components(fld, 0.0), "field" + GPU), (lambda: merge.components(np.zeros((4, 4, 4), np.float32), 0.0), "field" + GPU)]),
    (MG + "fill_field: ", [
        (lambda: merge.fill_field(fld, 0.0, "cavities"), "field" + GPU), (lambda: merge.fill_field(fld, nan, "none"), "field" + GPU),
        (lambda: merge._check_fill("fill_field", "none", allow_none=False), "mode must be one of 'cavities', 'outer', got 'none'"),
        (lambda: merge._check_fill("fill_field", 1, allow_none=False), "mode must be one of 'cavities', 'outer', got 1"),
    ]),
    (MG + "merge_tets: ", [
        (lambda: merge.merge_tets(v, e, fill="both"), FILL + "'both'"), (lambda: merge.merge_tets(v, e, fill=None), FILL + "None"),
        (lambda: merge.merge_tets(v, e, fill=2), FILL + "2"), (lambda: merge.merge_tets(None, e, grid=1, fill="both"), FILL + "'both'"),
        (lambda: merge.merge_tets(v, e, fill="outer"), "tet_v" + GPU), (lambda: merge.merge_tets(vn, e), "tet_v" + GPU),
        (lambda: merge.merge_tets(v, e, grid=1, bounds=3, level=nan, simplify=1), "tet_v" + GPU),
        (lambda: merge._check_simplify("merge_tets", 1, 32), "simplify must be None or an integer in 2 .. grid = 32, got 1"),
        (lambda: merge._check_simplify("merge_tets", 33, 32), "simplify must be None or an integer in 2 .. grid = 32, got 33"),
        (lambda: merge._check_simplify("merge_tets", 2.0, 32), "simplify must be None or an integer in 2 .. grid = 32, got 2.0"),
        (lambda: merge._check_simplify("merge_tets", True, 32), "simplify must be None or an integer in 2 .. grid = 32, got True"),
        (lambda: merge._check_level("merge_tets", nan), "level must be a number, not NaN"), (lambda: merge._check_level("merge_tets", "x"), "level must be a number, not NaN"),
    ]),
    (MG + "volume_iou: ", [
        (lambda: merge.volume_iou(fld, fld), "a must be a bool tensor"), (lambda: merge.volume_iou(None, occ), "a must be a bool tensor"),
        (lambda: merge.volume_iou(occ, fld), "b must be a bool tensor"), (lambda: merge.volume_iou(occ, occ[:2]), "b must have a's shape and device ((4, 4, 4), cpu), got (2, 4, 4), cpu"),
    ]),
    # ---- metrics: the device, dtype, shape, contiguity of each tensor in turn; the plain numbers where the function puts them ----
    (MT + "nearest_info: ", [
        (lambda: metrics.nearest_info(-1, 4), "n" + COUNT0 + "-1"), (lambda: metrics.nearest_info(2 ** 31, 4), "n" + COUNT0 + "2147483648"),
        (lambda: metrics.nearest_info(True, 4), "n" + COUNT0 + "True"), (lambda: metrics.nearest_info(1.0, 4), "n" + COUNT0 + "1.0"),
        (lambda: metrics.nearest_info(4, -1), "m" + COUNT0 + "-1"), (lambda: metrics.nearest_info(-1, -1), "n" + COUNT0 + "-1"),
        (lambda: metrics.nearest_info(0, 2 ** 31), "m" + COUNT0 + "2147483648"), (lambda: metrics.nearest_info(2 ** 31 - 1, 2 ** 31), "m" + COUNT0 + "2147483648"),
    ]),
    (MT + "sample_surface: ", [
        (lambda: metrics.sample_surface(v, f, 4), "v" + GPU), (lambda: metrics.sample_surface(None, f, 4), "v" + GPU), (lambda: metrics.sample_surface(vn, f, 4), "v" + GPU),
        (lambda: metrics.sample_surface(v.double()[:, :2], f.long(), -1, seed=0.5), "v" + GPU),
        (lambda: metrics._check_count("sample_surface", "n", 2 ** 31), "n" + COUNT0 + "2147483648"),
        (lambda: metrics._check_seed("sample_surface", 0.5), "seed must be an integer, got 0.5"), (lambda: metrics._check_seed("sample_surface", True), "seed must be an integer, got True"),
    ]),
    (MT + "nearest: ", [(lambda: metrics.nearest(pts, pts), "query" + GPU), (lambda: metrics.nearest(None, pts, ref_chunks=-1), "query" + GPU)]),
    (MT + "compare: ", [
        (lambda: metrics.compare(pts, samples), "a must be SurfaceSamples"), (lambda: metrics.compare(None, None, thresholds=(-1.0,)), "a must be SurfaceSamples"),
        (lambda: metrics.compare(samples, samples), "a.points" + GPU),
    ]),
    (MT + "compare_meshes: ", [
        (lambda: metrics.compare_meshes(v, f, v, f, n=0), "n must be an integer in 1 .. 2^31 - 1, got 0"),
        (lambda: metrics.compare_meshes(v, f, v, f, n=2 ** 31), "n must be an integer in 1 .. 2^31 - 1, got 2147483648"),
        (lambda: metrics.compare_meshes(v, f, v, f, n=True), "n must be an integer in 1 .. 2^31 - 1, got True"),
        (lambda: metrics.compare_meshes(v, f, v, f, n=1, seed=0.5), "seed must be an integer, got 0.5"),
        (lambda: metrics.compare_meshes(v, f, v, f, n=2 ** 31 - 1, seed="x"), "seed must be an integer, got 'x'"),
        (lambda: metrics.compare_meshes(v, f, v, f, n=0, seed=0.5, thresholds=(-1.0,)), "n must be an integer in 1 .. 2^31 - 1, got 0"),
        (lambda: metrics.compare_meshes(v, f, v, f, thresholds=(-1.0,)), "thresholds must be finite distances >= 0, got (-1.0,)"),
        (lambda: metrics.compare_meshes(v, f, v, f, thresholds=(0.1, inf)), "thresholds must be finite distances >= 0, got (0.1, inf)"),
        (lambda: metrics.compare_meshes(v, f, v, f, thresholds=3), "thresholds must be finite distances >= 0, got 3"),
        (lambda: metrics.compare_meshes(None, f, v, f, thresholds=(nan,)), "thresholds must be finite distances >= 0, got (nan,)"),
        (lambda: metrics.compare_meshes(v, f, v, f, n=10), "v_a" + GPU), (lambda: metrics.compare_meshes(None, None, None, None), "v_a" + GPU),
    ]),
    # ---- simplify: the plain numbers, then what is wrong with a tensor (type, dtype, shape) before where it lives ----
    (SP + "simplify: ", [
        (lambda: simplify.simplify(v, f, 0), CELLS + "0"), (lambda: simplify.simplify(v, f, 1025), CELLS + "1025"), (lambda: simplify.simplify(v, f, 2.0), CELLS + "2.0"),
        (lambda: simplify.simplify(v, f, True), CELLS + "True"), (lambda: simplify.simplify(v, f, 1), "v" + GPU), (lambda: simplify.simplify(v, f, 1024), "v" + GPU),
        (lambda: simplify.simplify(v, f, 0, bounds=3, placement="median", stabilise=-1.0), CELLS + "0"),
        (lambda: simplify.simplify(v, f, 4, placement="median"), "placement must be one of 'quadric', 'mean', got 'median'"),
        (lambda: simplify.simplify(v, f, 4, placement=None), "placement must be one of 'quadric', 'mean', got None"),
        (lambda: simplify.simplify(v, f, 4, placement=0, stabilise=-1.0, bounds=3), "placement must be one of 'quadric', 'mean', got 0"),
        (lambda: simplify.simplify(v, f, 4, stabilise=-1.0), "stabilise must be a finite number >= 0, got -1.0"),
        (lambda: simplify.simplify(v, f, 4, stabilise=nan), "stabilise must be a finite number >= 0, got nan"),
        (lambda: simplify.simplify(v, f, 4, stabilise=True), "stabilise must be a finite number >= 0, got True"),
        (lambda: simplify.simplify(v, f, 4, stabilise="x", bounds=3), "stabilise must be a finite number >= 0, got 'x'"),
        (lambda: simplify.simplify(None, f, 4), "v" + GPU + ", got NoneType"), (lambda: simplify.simplify(vn, f, 4), "v" + GPU + ", got ndarray"),
        (lambda: simplify.simplify(v.double(), f, 4), "v must be float32, got float64"), (lambda: simplify.simplify(v[:, :2], f, 4), ROWS_V + "(4, 2)"),
        (lambda: simplify.simplify(v.reshape(-1), f, 4), ROWS_V + "(12,)"), (lambda: simplify.simplify(v, None, 4), "faces" + GPU + ", got NoneType"),
        (lambda: simplify.simplify(v, f.long(), 4), "faces must be int32, got int64"), (lambda: simplify.simplify(v, f.reshape(-1), 4), ROWS_F + "(6,)"),
        (lambda: simplify.simplify(v.double(), f.reshape(-1), 4), "v must be float32, got float64"), (lambda: simplify.simplify(v[:, :2].double(), f, 4), "v must be float32, got float64"),
        (lambda: simplify.simplify(v, f, 4), "v" + GPU), (lambda: simplify.simplify(v, f, 4, bounds=UNIT), "v" + GPU),
    ] + bounds_rows(lambda b: simplify.simplify(None, f, 4, bounds=b), BAD_BOUNDS + [(OVERFLOW, OVERFLOW_TEXT), TINY])),
    (SP + "run_lengths: ", [
        (lambda: simplify.run_lengths(v, f, 0), CELLS + "0"), (lambda: simplify.run_lengths(v, f, 1025, bounds=3), CELLS + "1025"),
        (lambda: simplify.run_lengths(v, f.long(), 4), "faces must be int32, got int64"), (lambda: simplify.run_lengths(v, f, 4), "v" + GPU),
    ] + bounds_rows(lambda b: simplify.run_lengths(None, f, 4, bounds=b), BAD_BOUNDS[:2] + [TINY])),
    (SP + "edge_stats: ", [
        (lambda: simplify.edge_stats(None), "faces" + GPU + ", got NoneType"), (lambda: simplify.edge_stats(f.long()), "faces must be int32, got int64"),
        (lambda: simplify.edge_stats(f[:, :2]), ROWS_F + "(2, 2)"), (lambda: simplify.edge_stats(f), "faces" + GPU),
    ]),
    # ---- voxelize: as simplify ----
    (VX + "workspace_bytes: ", [
        (lambda: voxelize.workspace_bytes(0), G512 + "0"), (lambda: voxelize.workspace_bytes(513), G512 + "513"), (lambda: voxelize.workspace_bytes(True), G512 + "True"),
        (lambda: voxelize.workspace_bytes(1.0), G512 + "1.0"),
    ]),
    (VX + "winding: ", [
        (lambda: voxelize.winding(v, f, 0, UNIT), G512 + "0"), (lambda: voxelize.winding(v, f, 513, UNIT), G512 + "513"), (lambda: voxelize.winding(v, f, 0, 3, axis=3), G512 + "0"),
        (lambda: voxelize.winding(v, f, 1, UNIT), "v" + GPU), (lambda: voxelize.winding(v, f, 512, UNIT), "v" + GPU),
        (lambda: voxelize.winding(v, f, 8, UNIT, axis=3), "axis must be 0, 1 or 2, got 3"), (lambda: voxelize.winding(v, f, 8, UNIT, axis=-1), "axis must be 0, 1 or 2, got -1"),
        (lambda: voxelize.winding(v, f, 8, UNIT, axis=True), "axis must be 0, 1 or 2, got True"), (lambda: voxelize.winding(None, f, 8, UNIT, axis=0.0), "axis must be 0, 1 or 2, got 0.0"),
        (lambda: voxelize.winding(v, f, 8, UNIT, axis=2), "v" + GPU), (lambda: voxelize.winding(None, f, 8, UNIT), "v" + GPU + ", got NoneType"),
        (lambda: voxelize.winding(vn, f, 8, UNIT), "v" + GPU + ", got ndarray"), (lambda: voxelize.winding(v.double(), f, 8, UNIT), "v must be float32, got float64"),
        (lambda: voxelize.winding(v[:, :2], f, 8, UNIT), ROWS_V + "(4, 2)"), (lambda: voxelize.winding(v, f.long(), 8, UNIT), "faces must be int32, got int64"),
        (lambda: voxelize.winding(v, f[:, :2], 8, UNIT), "faces must be [N, 3] with N <= 2147483647, got (2, 2)"),
        (lambda: voxelize.winding(v.double(), None, 8, UNIT), "v must be float32, got float64"),
    ] + bounds_rows(lambda b: voxelize.winding(None, f, 8, b, axis=3), BAD_BOUNDS + [(OVERFLOW, OVERFLOW_TEXT), TINY])),
    (VX + "occupancy: ", [
        (lambda: voxelize.occupancy(v, f, 0, UNIT, rule="even"), G512 + "0"), (lambda: voxelize.occupancy(v, f, 8, (1.0, 1.0), rule="even"), BOUNDS + "(1.0, 1.0)"),
        (lambda: voxelize.occupancy(v, f, 8, UNIT, rule="even"), RULE + "'even'"), (lambda: voxelize.occupancy(v, f, 8, UNIT, rule=0, rays=2), RULE + "0"),
        (lambda: voxelize.occupancy(v, f, 8, UNIT, rays=2), "rays must be 1 or 3, got 2"), (lambda: voxelize.occupancy(v, f, 8, UNIT, rays=3.0), "rays must be 1 or 3, got 3.0"),
        (lambda: voxelize.occupancy(None, f, 8, UNIT, rays=True), "rays must be 1 or 3, got True"), (lambda: voxelize.occupancy(v, f, 8, UNIT, rays=1), "v" + GPU),
        (lambda: voxelize.occupancy(v.double(), f, 8, UNIT), "v must be float32, got float64"), (lambda: voxelize.occupancy(v, f.long(), 8, UNIT), "faces must be int32, got int64"),
        (lambda: voxelize.occupancy(v, f[:, :2], 8, UNIT), "faces must be [N, 3] with N <= 2147483647, got (2, 2)"), (lambda: voxelize.occupancy(v, f, 8, UNIT), "v" + GPU),
    ]),
    (VX + "mesh_volume_iou: ", [
        (lambda: voxelize.mesh_volume_iou(v, f, v, f, 0, UNIT, rule=0), G512 + "0"), (lambda: voxelize.mesh_volume_iou(v, f, v, f, 8, UNIT, rule=0, rays=2), RULE + "0"),
        (lambda: voxelize.mesh_volume_iou(v, f, v, f, 8, 3, rays=2), "rays must be 1 or 3, got 2"), (lambda: voxelize.mesh_volume_iou(None, f, v, f, 8, (1.0, 1.0)), BOUNDS + "(1.0, 1.0)"),
        (lambda: voxelize.mesh_volume_iou(v, f, v, f, 8, OVERFLOW), BOUNDS + OVERFLOW_TEXT),
        (lambda: voxelize.mesh_volume_iou(None, f, v, f, 8, UNIT), "v_a" + GPU + ", got NoneType"), (lambda: voxelize.mesh_volume_iou(v.double(), f, v, f, 8, UNIT), "v_a must be float32, got float64"),
        (lambda: voxelize.mesh_volume_iou(v, f.long(), v, f, 8, UNIT), "f_a must be int32, got int64"),
        (lambda: voxelize.mesh_volume_iou(v, f[:, :2], v, f, 8, UNIT), "f_a must be [N, 3] with N <= 2147483647, got (2, 2)"),
        (lambda: voxelize.mesh_volume_iou(v, f, v, f, 8, UNIT), "v_a" + GPU), (lambda: voxelize.mesh_volume_iou(v, f, v.double(), None, 8, UNIT), "v_a" + GPU),
    ]),
]


def test_python_messages_without_a_device():
    assert mismatches(CPU_TABLES) == []
    # both ends of a range pass where nothing after them needs a device
    assert spheres_init.voxel_centres(1).shape == (1,) and spheres_init.voxel_centres(512).shape == (512,)
    assert merge.default_level(2, UNIT) < 0 and merge.default_level(512, UNIT) < 0
    assert metrics.nearest_info(0, 0).auto_chunks == 1 and metrics.nearest_info(2 ** 31 - 1, 2 ** 31 - 1).auto_chunks >= 1
    assert voxelize.workspace_bytes(1) == 6144 + 3 * 2 * 4 and voxelize.workspace_bytes(512) > 0
    assert merge._check_simplify("merge_tets", 2, 32) == 2 and merge._check_simplify("merge_tets", 32, 32) == 32
    assert metrics._check_count("nearest_info", "n", np.int64(7)) == 7 and metrics._check_seed("sample_surface", -1) == 2 ** 64 - 1


def test_bounds_whose_difference_overflows_are_refused_by_the_sphere_initialisation():
    """``hi - lo = inf`` with both ends finite: merge, simplify and voxelize always refused it (the rows above); the sphere
    initialisation computed with ``h = inf`` (``voxel_centres`` returned inf and nan) or left the refusal to the library."""
    assert mismatches([
        (SI + "voxel_centres: ", [(lambda: spheres_init.voxel_centres(4, OVERFLOW), BOUNDS + OVERFLOW_TEXT)]),
        (SI + "visual_hull: ", [(lambda: spheres_init.visual_hull(alpha, mvp, bounds=OVERFLOW), BOUNDS + OVERFLOW_TEXT)]),
        (SI + "init_spheres: ", [(lambda: spheres_init.init_spheres(alpha, mvp, 2, bounds=OVERFLOW), BOUNDS + OVERFLOW_TEXT)]),
    ]) == []


# ---------------------------------------------------------------- Python, past the first check: tensors on the device ----------------------------------------------------------------
def _gpu_tables():
    d = lambda t: t.cuda()
    gv, gf, ge, gfld, gpts, galpha, gmvp, gocc = (d(t) for t in (v, f, e, fld, pts, alpha, mvp, occ))
    gd2 = gocc.int()
    gs = metrics.SurfaceSamples(gpts, gpts, None)
    SS = metrics.SurfaceSamples
    ROWS = " must be [N, 3] with N <= 2^31 - 1, got "
    CH = "channel must be an integer in 0 .. 0, got "
    SIMPLIFY = "simplify must be None or an integer in 2 .. grid = 4, got "
    CHUNKS = "ref_chunks must be 0 (automatic) or an integer in 1 .. min(M, 65535) = 5, got "
    FIELD = "field must be [G, G, G] with G in 2 .. 512, got "
    return [
        (SI + "visual_hull: ", [
            (lambda: spheres_init.visual_hull(galpha.double(), mvp), "alpha must be float32, got float64"),
            (lambda: spheres_init.visual_hull(galpha[0], mvp), "alpha must be [B, H, W, C] with B, C >= 1 and H, W in 1 .. 8192, got (8, 8, 1)"),
            (lambda: spheres_init.visual_hull(galpha[:0], gmvp), "alpha must be [B, H, W, C] with B, C >= 1 and H, W in 1 .. 8192, got (0, 8, 8, 1)"),
            (lambda: spheres_init.visual_hull(galpha, mvp), "mvp" + GPU), (lambda: spheres_init.visual_hull(galpha, None), "mvp" + GPU),
            (lambda: spheres_init.visual_hull(galpha, gmvp.double()), "mvp must be float32, got float64"),
            (lambda: spheres_init.visual_hull(galpha, gmvp[0]), "mvp must be [1, 4, 4] (one matrix per view of alpha), got (4, 4)"),
            (lambda: spheres_init.visual_hull(galpha, gmvp, channel=1), CH + "1"), (lambda: spheres_init.visual_hull(galpha, gmvp, channel=-1), CH + "-1"),
            (lambda: spheres_init.visual_hull(galpha, gmvp, channel=True), CH + "True"), (lambda: spheres_init.visual_hull(galpha, gmvp, channel=0.0, threshold=nan), CH + "0.0"),
            (lambda: spheres_init.visual_hull(galpha, gmvp, threshold=nan), "threshold is NaN"),
            (lambda: spheres_init.visual_hull(galpha.transpose(1, 2), gmvp, grid=4, threshold=nan), "threshold is NaN"),
        ]),
        (SI + "distance_transform_sq: ", [
            (lambda: spheres_init.distance_transform_sq(gfld), "mask must be bool, got float32"),
            (lambda: spheres_init.distance_transform_sq(gocc[:, :, :2]), "mask must be [G, G, G] with G in 1 .. 512, got (4, 4, 2)"),
            (lambda: spheres_init.distance_transform_sq(gocc[0]), "mask must be [G, G, G] with G in 1 .. 512, got (4, 4)"),
        ]),
        (SI + "greedy_cover: ", [
            (lambda: spheres_init.greedy_cover(gocc, occ.int(), 1), "d2" + GPU), (lambda: spheres_init.greedy_cover(gocc, gocc.long(), 1), "d2 must be int32, got int64"),
            (lambda: spheres_init.greedy_cover(gocc, gd2[:2, :2, :2], 1), "d2 must be [4, 4, 4], got (2, 2, 2)"),
            (lambda: spheres_init.greedy_cover(gocc, gd2, -1, bounds=(1.0, 1.0)), BOUNDS + "(1.0, 1.0)"), (lambda: spheres_init.greedy_cover(gocc, gd2, -1), NSPH + "-1"),
            (lambda: spheres_init.greedy_cover(gocc, gd2, (1 << 20) + 1), NSPH + "1048577"), (lambda: spheres_init.greedy_cover(gocc, gd2, 1.5), NSPH + "1.5"),
            (lambda: spheres_init.greedy_cover(gocc, gd2, 0, min_radius=-1.0), "min_radius must be finite and not negative, got -1.0"),
            (lambda: spheres_init.greedy_cover(gocc, gd2, 1 << 20, shrink=0.0), "shrink must be finite and positive, got 0.0"),
        ]),
        (SI + "cover_occupancy: ", [
            (lambda: spheres_init.cover_occupancy(gd2, 3), "occ must be bool, got int32"), (lambda: spheres_init.cover_occupancy(gocc, -1, bounds=3), BOUNDS + "3"),
            (lambda: spheres_init.cover_occupancy(gocc, -1), NSPH + "-1"), (lambda: spheres_init.cover_occupancy(gocc, 2, shrink=nan), "shrink must be finite and positive, got nan"),
        ]),
        (SI + "init_spheres: ", [(lambda: spheres_init.init_spheres(galpha, gmvp, 2, channel=1), CH + "1")]),
        (MG + "default_bounds: ", [(lambda: merge.default_bounds(gv.double(), 8), "tet_v must be float32, got float64")]),
        (MG + "union_field: ", [
            (lambda: merge.union_field(gv.double(), ge, 8, UNIT), "tet_v must be float32, got float64"), (lambda: merge.union_field(gv[:, :2], ge, 8, UNIT), "tet_v must be [V, 3], got (4, 2)"),
            (lambda: merge.union_field(gv, e, 8, UNIT), "elem" + GPU), (lambda: merge.union_field(gv, None, 8, UNIT), "elem" + GPU),
            (lambda: merge.union_field(gv, ge.long(), 8, UNIT), "elem must be int32, got int64"), (lambda: merge.union_field(gv, ge[:, :3], 8, UNIT), "elem must be [T, 4] with T <= 2^30, got (1, 3)"),
            (lambda: merge.union_field(gv[:, :2], ge.long(), 1, UNIT), "tet_v must be [V, 3], got (4, 2)"),
            (lambda: merge.union_field(gv, ge, 1, (1.0, 1.0)), G2 + "1"), (lambda: merge.union_field(gv, ge, 513, UNIT), G2 + "513"), (lambda: merge.union_field(gv, ge, True, UNIT), G2 + "True"),
        ] + bounds_rows(lambda b: merge.union_field(gv, ge, 2, b), BAD_BOUNDS + [(OVERFLOW, OVERFLOW_TEXT)])),
        (MG + "extract_surface: ", [
            (lambda: merge.extract_surface(gfld.double(), UNIT, 0.0), "field must be float32, got float64"), (lambda: merge.extract_surface(gfld[:, :, :2], UNIT, 0.0), FIELD + "(4, 4, 2)"),
            (lambda: merge.extract_surface(gfld[:1, :1, :1], UNIT, 0.0), FIELD + "(1, 1, 1)"), (lambda: merge.extract_surface(gfld, (1.0, 1.0), nan), BOUNDS + "(1.0, 1.0)"),
            (lambda: merge.extract_surface(gfld, UNIT, nan), "level must be a number, not NaN"), (lambda: merge.extract_surface(gfld, UNIT, "x"), "level must be a number, not NaN"),
        ]),
        (MG + "occupancy: ", [(lambda: merge.occupancy(gfld[0], 0.0), FIELD + "(4, 4)"), (lambda: merge.occupancy(gfld, nan), "level must be a number, not NaN")]),
        (MG + "components: ", [(lambda: merge.components(gfld.half(), 0.0), "field must be float32, got float16"), (lambda: merge.components(gfld, nan), "level must be a number, not NaN")]),
        (MG + "fill_field: ", [
            (lambda: merge.fill_field(gfld, nan, "none"), "level must be a number, not NaN"), (lambda: merge.fill_field(gfld, 0.0, "none"), "mode must be one of 'cavities', 'outer', got 'none'"),
            (lambda: merge.fill_field(gfld, 0.0, None), "mode must be one of 'cavities', 'outer', got None"),
        ]),
        (MG + "merge_tets: ", [
            (lambda: merge.merge_tets(gv, e, grid=1), "elem" + GPU), (lambda: merge.merge_tets(gv, ge, grid=1, simplify=1), G2 + "1"),
            (lambda: merge.merge_tets(gv, ge, grid=4, bounds=3, simplify=1), SIMPLIFY + "1"), (lambda: merge.merge_tets(gv, ge, grid=4, bounds=UNIT, simplify=5), SIMPLIFY + "5"),
            (lambda: merge.merge_tets(gv, ge, grid=4, bounds=UNIT, simplify=True), SIMPLIFY + "True"), (lambda: merge.merge_tets(gv, ge, grid=4, bounds=3, simplify=2), BOUNDS + "3"),
            (lambda: merge.merge_tets(gv, ge, grid=4, bounds=(1.0, -1.0), simplify=4, level=nan), BOUNDS + "(1.0, -1.0)"),
            (lambda: merge.merge_tets(gv, ge, grid=4, bounds=OVERFLOW), BOUNDS + OVERFLOW_TEXT), (lambda: merge.merge_tets(gv, ge, grid=4, bounds=UNIT, level=nan), "level must be a number, not NaN"),
        ]),
        (MG + "volume_iou: ", [(lambda: merge.volume_iou(gocc, occ), "b must have a's shape and device ((4, 4, 4), cuda:0), got (4, 4, 4), cpu")]),
        (MT + "sample_surface: ", [
            (lambda: metrics.sample_surface(gv.double(), gf, 4), "v must be float32, got float64"), (lambda: metrics.sample_surface(gv[:, :2], gf, 4), "v" + ROWS + "(4, 2)"),
            (lambda: metrics.sample_surface(gv.reshape(-1), gf, 4), "v" + ROWS + "(12,)"), (lambda: metrics.sample_surface(gv.T.contiguous().T, gf, 4), "v must be contiguous"),
            (lambda: metrics.sample_surface(gv.double()[:, :2], f, 4), "v must be float32, got float64"),
            (lambda: metrics.sample_surface(gv, f, 4), "faces" + GPU), (lambda: metrics.sample_surface(gv, gf.long(), 4), "faces must be int32, got int64"),
            (lambda: metrics.sample_surface(gv, gf[:, :2], 4), "faces" + ROWS + "(2, 2)"), (lambda: metrics.sample_surface(gv, gf.T.contiguous().T, -1), "faces must be contiguous"),
            (lambda: metrics.sample_surface(gv, gf, -1, seed=0.5), "n" + COUNT0 + "-1"), (lambda: metrics.sample_surface(gv, gf, 2 ** 31), "n" + COUNT0 + "2147483648"),
            (lambda: metrics.sample_surface(gv, gf, True), "n" + COUNT0 + "True"), (lambda: metrics.sample_surface(gv, gf, 4.0), "n" + COUNT0 + "4.0"),
            (lambda: metrics.sample_surface(gv, gf, 0, seed=0.5), "seed must be an integer, got 0.5"), (lambda: metrics.sample_surface(gv, gf, 2 ** 31 - 1, seed="x"), "seed must be an integer, got 'x'"),
            (lambda: metrics.sample_surface(gv, gf[:0], 4), "faces holds no triangle"),
        ]),
        (MT + "nearest: ", [
            (lambda: metrics.nearest(gpts.reshape(-1), gpts), "query" + ROWS + "(15,)"), (lambda: metrics.nearest(gpts, pts), "ref" + GPU),
            (lambda: metrics.nearest(gpts, gpts.double()), "ref must be float32, got float64"), (lambda: metrics.nearest(gpts, gpts[:, :2]), "ref" + ROWS + "(5, 2)"),
            (lambda: metrics.nearest(gpts, gpts[:0], ref_chunks=-1), "ref holds no point"), (lambda: metrics.nearest(gpts, gpts, ref_chunks=-1), CHUNKS + "-1"),
            (lambda: metrics.nearest(gpts, gpts, ref_chunks=6), CHUNKS + "6"), (lambda: metrics.nearest(gpts, gpts, ref_chunks=True), CHUNKS + "True"),
            (lambda: metrics.nearest(gpts, gpts, ref_chunks=1.0), CHUNKS + "1.0"),
        ]),
        (MT + "compare: ", [
            (lambda: metrics.compare(SS(gpts, pts, None), gs), "a.normals" + GPU), (lambda: metrics.compare(SS(gpts, gpts[:4], None), gs), "a.normals must have a.points' rows (5), got 4"),
            (lambda: metrics.compare(SS(gpts[:0], gpts[:0], None), gs), "a.points holds no sample"), (lambda: metrics.compare(gs, gpts), "b must be SurfaceSamples"),
            (lambda: metrics.compare(gs, samples), "b.points" + GPU), (lambda: metrics.compare(gs, SS(gpts, gpts.double(), None)), "b.normals must be float32, got float64"),
            (lambda: metrics.compare(gs, gs, thresholds=(-1.0,)), "thresholds must be finite distances >= 0, got (-1.0,)"),
        ]),
        (MT + "compare_meshes: ", [
            (lambda: metrics.compare_meshes(gv, gf.long(), gv, gf), "f_a must be int32, got int64"), (lambda: metrics.compare_meshes(gv, gf, v, gf), "v_b" + GPU),
            (lambda: metrics.compare_meshes(gv, gf, gv, gf[:, :2]), "f_b" + ROWS + "(2, 2)"),
        ]),
        (SP + "simplify: ", [(lambda: simplify.simplify(gv, f, 4), "faces" + GPU), (lambda: simplify.simplify(v, gf, 4), "v" + GPU), (lambda: simplify.simplify(gv.double(), f, 4), "v must be float32, got float64")]),
        (SP + "run_lengths: ", [(lambda: simplify.run_lengths(gv, f, 4), "faces" + GPU)]),
        (VX + "winding: ", [(lambda: voxelize.winding(gv, f, 8, UNIT), "faces" + GPU), (lambda: voxelize.winding(v, gf, 8, UNIT), "v" + GPU)]),
        (VX + "occupancy: ", [(lambda: voxelize.occupancy(gv, f, 8, UNIT), "faces" + GPU)]),
        (VX + "mesh_volume_iou: ", [
            (lambda: voxelize.mesh_volume_iou(gv, f, gv, gf, 8, UNIT), "f_a" + GPU), (lambda: voxelize.mesh_volume_iou(gv, gf, v, gf, 8, UNIT), "v_b" + GPU),
            (lambda: voxelize.mesh_volume_iou(gv, gf, gv, f, 8, UNIT), "f_b" + GPU), (lambda: voxelize.mesh_volume_iou(gv, gf, gv.double(), f, 8, UNIT), "v_b must be float32, got float64"),
        ]),
    ], (gocc, gd2)


@gpu
def test_python_messages_past_the_device_check():
    tables, _ = _gpu_tables()
    assert mismatches(tables) == []


@gpu
def test_overflowing_bounds_are_refused_past_the_device_check():
    """The rest of the one deliberate change: both calls also carry a bad ``n_spheres``, which the bounds now come before."""
    _, (gocc, gd2) = _gpu_tables()
    assert mismatches([
        (SI + "greedy_cover: ", [(lambda: spheres_init.greedy_cover(gocc, gd2, -1, bounds=OVERFLOW), BOUNDS + OVERFLOW_TEXT)]),
        (SI + "cover_occupancy: ", [(lambda: spheres_init.cover_occupancy(gocc, -1, bounds=OVERFLOW), BOUNDS + OVERFLOW_TEXT)]),
    ]) == []


# ---------------------------------------------------------------- what the checks hand on: a copy where the layout is not the kernels' ----------------------------------------------------------------
# spheres_init, merge, simplify and voxelize copy a tensor that is not contiguous and detach one that carries a gradient (metrics
# refuses the former: the table above).  One tetrahedron on grid 4 reaches every kernel; the outputs must not depend on either.
TET_V = np.array([[-0.5, -0.5, -0.5], [0.6, -0.5, -0.5], [-0.5, 0.6, -0.5], [-0.5, -0.5, 0.6]], np.float32)      # positive signed volume
TET_ELEM = np.array([[0, 1, 2, 3]], np.int32)
TET_FACES = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)                                      # normals point outwards


def _strided(t):
    """The same values behind a last-axis stride of 2."""
    buf = t.new_zeros(t.shape[:-1] + (2 * t.shape[-1],))
    buf[..., ::2] = t
    view = buf[..., ::2]
    assert not view.is_contiguous() and torch.equal(view, t)
    return view


def _with_grad(t):
    return t.clone().requires_grad_(True)


def _bits(out):
    """Every tensor of a result as (dtype, shape, bytes); everything else as it is."""
    if isinstance(out, torch.Tensor):
        out = out.detach().cpu().numpy()
    if isinstance(out, np.ndarray):
        return (str(out.dtype), out.shape, out.tobytes())
    if hasattr(out, "__dataclass_fields__"):
        return tuple(_bits(getattr(out, k)) for k in out.__dataclass_fields__)
    if isinstance(out, (tuple, list)):
        return tuple(_bits(x) for x in out)
    return out


def _tetrahedron():
    return tuple(torch.from_numpy(a).cuda() for a in (TET_V, TET_ELEM, TET_FACES))


@gpu
def test_spheres_init_copies_views_and_detaches():
    from tssplat_amd import scenes
    a = np.zeros((1, 8, 8, 1), np.float32)
    a[0, 1:7, 2:6, 0] = 1.0                                              # not symmetric in H and W: a transposed read would show
    a, m = torch.from_numpy(a).cuda(), torch.from_numpy(scenes.orbit_mvps(1).astype(np.float32)).cuda()
    a_view = a.transpose(1, 2).contiguous().transpose(1, 2)
    assert not a_view.is_contiguous() and torch.equal(a_view, a)
    hull = spheres_init.visual_hull(a, m, grid=4)
    want = _bits(hull)
    for alpha_, mvp_ in [(a_view, _strided(m)), (_with_grad(a), _with_grad(m))]:
        assert _bits(spheres_init.visual_hull(alpha_, mvp_, grid=4)) == want
    mask = torch.from_numpy(np.arange(64).reshape(4, 4, 4) % 5 != 0).cuda()
    d2 = spheres_init.distance_transform_sq(mask)
    assert _bits(spheres_init.distance_transform_sq(_strided(mask))) == _bits(d2)
    cover = _bits(spheres_init.greedy_cover(mask, d2, 3))
    assert _bits(spheres_init.greedy_cover(_strided(mask), _strided(d2), 3)) == cover and len(cover[0][2]) > 0
    assert _bits(spheres_init.cover_occupancy(_strided(mask), 3)) == _bits(spheres_init.cover_occupancy(mask, 3))


@gpu
def test_merge_copies_views_and_detaches():
    tv, te, _ = _tetrahedron()
    field = merge.union_field(tv, te, 4, UNIT)
    assert (field > 0).any() and (field < 0).any()
    merged = merge.merge_tets(tv, te, grid=4, bounds=UNIT)
    assert merged.faces.shape[0] > 0
    for tv_, te_ in [(_strided(tv), _strided(te)), (_with_grad(tv), te)]:
        assert _bits(merge.union_field(tv_, te_, 4, UNIT)) == _bits(field)
        assert _bits(merge.merge_tets(tv_, te_, grid=4, bounds=UNIT)) == _bits(merged)
    for field_ in (_strided(field), _with_grad(field)):
        assert _bits(merge.extract_surface(field_, UNIT, 0.0)) == _bits(merge.extract_surface(field, UNIT, 0.0))
        assert _bits(merge.components(field_, 0.0)) == _bits(merge.components(field, 0.0))
        assert _bits(merge.fill_field(field_, 0.0, "outer")) == _bits(merge.fill_field(field, 0.0, "outer"))


@gpu
def test_simplify_copies_views_and_detaches():
    tv, _, tf = _tetrahedron()
    want = simplify.simplify(tv, tf, 2, bounds=UNIT)
    assert want.faces.shape[0] > 0
    for tv_, tf_ in [(_strided(tv), _strided(tf)), (_with_grad(tv), tf)]:
        assert _bits(simplify.simplify(tv_, tf_, 2, bounds=UNIT)) == _bits(want)
        assert _bits(simplify.run_lengths(tv_, tf_, 2, UNIT)) == _bits(simplify.run_lengths(tv, tf, 2, UNIT))
    assert _bits(simplify.edge_stats(_strided(tf))) == _bits(simplify.edge_stats(tf)) and simplify.edge_stats(tf).closed


@gpu
def test_voxelize_copies_views_and_detaches():
    tv, _, tf = _tetrahedron()
    wind, occ3 = voxelize.winding(tv, tf, 4, UNIT), voxelize.occupancy(tv, tf, 4, UNIT)
    assert occ3.occ.any() and not occ3.occ.all() and wind.open_columns == 0
    for tv_, tf_ in [(_strided(tv), _strided(tf)), (_with_grad(tv), tf)]:
        assert _bits(voxelize.winding(tv_, tf_, 4, UNIT)) == _bits(wind)
        assert _bits(voxelize.occupancy(tv_, tf_, 4, UNIT)) == _bits(occ3)
        assert _bits(voxelize.mesh_volume_iou(tv_, tf_, tv, tf, 4, UNIT)["a"]) == _bits(occ3)


# ---------------------------------------------------------------- the C entry points ----------------------------------------------------------------
p, q_, odd, half = 0x1000, 0x2000, 0x1002, 0x1004      # "not null"; never dereferenced.  odd: not 4-byte aligned; half: not 8-byte aligned
big = 2 ** 31
GRID1 = "grid out of range (1 .. 512)"
GRID2 = "grid out of range (2 .. 512)"
CUBE = "lo must be below hi, both finite"
CUBE_CELLS = "lo / hi must be finite with lo < hi and (hi - lo) / cells > 0"
CUBE_GRID = "lo / hi must be finite with lo < hi and (hi - lo) / grid > 0"
IMAGE = "batch / height / width out of range (0 .. 8192 pixels per side)"
LEVEL = "level is NaN"
NV_ELEM = "n_vertices out of range (0 .. 2^31 - 1: elem holds 32-bit indices)"
NV_FACES = "n_vertices out of range (0 .. 2^31 - 1: faces holds 32-bit indices)"
NT_SIMPLIFY = "n_triangles out of range (0 .. (2^31 - 1) / 3: three record slots per triangle)"
NULL = " is null"
A4, A8 = " must be 4-byte aligned", " must be 8-byte aligned"


def _lib():
    return _capi.load()


def carve(alpha=p, batch=2, height=8, width=8, channels=2, channel=1, mvp=p, grid=8, lo=-1.0, hi=1.0, bits=p, hull=p):
    return _lib().tsamd_hull_carve(alpha, batch, height, width, channels, channel, 0.5, mvp, grid, lo, hi, bits, hull, None)


def edt(mask=p, grid=8, ws=p, d2=p, status=p):
    return _lib().tsamd_edt_squared(mask, grid, ws, d2, status, None)


def cover(hull=p, d2=p, grid=8, n=4, s2=1.0, hs2=1.0, m2=0.0, ws=p, unc=p, flat=p, q=p, count=p):
    return _lib().tsamd_greedy_cover(hull, d2, grid, n, s2, hs2, m2, ws, unc, flat, q, count, None)


def field(tet_v=p, nv=8, elem=p, nt=4, grid=8, lo=-1.0, hi=1.0, out=p):
    return _lib().tsamd_union_field(tet_v, nv, elem, nt, grid, lo, hi, out, None)


def count(f=p, grid=8, level=0.0, vmask=p, vcount=p, tcount=p, flag=p):
    return _lib().tsamd_surface_count(f, grid, level, vmask, vcount, tcount, flag, None)


def emit(f=p, grid=8, lo=-1.0, hi=1.0, level=0.0, vmask=p, voff=p, toff=p, nv=3, nt=1, v=p, faces=p):
    return _lib().tsamd_surface_emit(f, grid, lo, hi, level, vmask, voff, toff, nv, nt, v, faces, None)


def comps(f=p, grid=8, level=0.0, label=p, status=p):
    return _lib().tsamd_grid_components(f, grid, level, label, status, None)


def fill(f=p, grid=8, level=0.0, mode=1, work=p, out=q_, stats=p):
    return _lib().tsamd_field_fill(f, grid, level, mode, work, out, stats, None)


def near(q=p, n=4, r=p, m=4, chunks=0, work=p, d2=p, idx=p):
    return _lib().tsamd_nearest_points(q, n, r, m, chunks, work, d2, idx, None)


def weights(v=p, nv=3, f=p, nt=1, prefix=p, work=p, phase=0):
    return _lib().tsamd_sample_surface(phase, v, nv, f, nt, prefix, work, 0, 0, None, None, None, None)


def draw(v=p, nv=3, f=p, nt=1, prefix=p, n=4, pts=p, nrm=p, tri=p):
    return _lib().tsamd_sample_surface(1, v, nv, f, nt, prefix, None, n, 0, pts, nrm, tri, None)


def info(n=4, m=4, out=(1, 1, 1, 1)):
    slots = [C.c_int32() for _ in range(4)]
    return _lib().tsamd_nearest_points_info(n, m, *(C.byref(s) if keep else None for s, keep in zip(slots, out)))


def keys(v=p, nv=3, f=p, nt=1, cells=4, lo=0.0, hi=1.0, vkey=p, rec=p, state=p):
    return _lib().tsamd_simplify_keys(v, nv, f, nt, cells, lo, hi, vkey, rec, state, None)


def cells_(v=p, nv=3, f=p, nt=1, cells=4, lo=0.0, hi=1.0, placement=0, stab=0.0, vkey=p, rec=p, perm=p, pos=p, head=p, run=p, status=p):
    return _lib().tsamd_simplify_cells(v, nv, f, nt, cells, lo, hi, placement, stab, vkey, rec, perm, pos, head, run, status, None)


def faces_(run=p, state=p, nt=1, tri=p, ab=p, c=p):
    return _lib().tsamd_simplify_faces(run, state, nt, tri, ab, c, None)


def dedupe(tri=p, order=p, nt=1, keep=p, used=p, status=p):
    return _lib().tsamd_simplify_dedupe(tri, order, nt, keep, used, status, None)


def wind(v=p, nv=8, faces=p, nt=4, grid=8, lo=-1.0, hi=1.0, axis=0, ws=p, w=p, stats=p):
    return _lib().tsamd_voxel_winding(v, nv, faces, nt, grid, lo, hi, axis, ws, w, stats, None)


def occ_(v=p, nv=8, faces=p, nt=4, grid=8, lo=-1.0, hi=1.0, rule=0, rays=3, ws=p, out=p, stats=p):
    return _lib().tsamd_voxel_occupancy(v, nv, faces, nt, grid, lo, hi, rule, rays, ws, out, stats, None)


C_CASES = [
    # ---- tsamd_hull_carve, _edt_squared, _greedy_cover (the lists of tests/test_spheres_init.py) ----
    (carve, dict(grid=0), GRID1), (carve, dict(grid=513), GRID1), (carve, dict(grid=-3), GRID1), (carve, dict(batch=-1), IMAGE), (carve, dict(height=-1), IMAGE),
    (carve, dict(width=-1), IMAGE), (carve, dict(width=8193), IMAGE), (carve, dict(height=0), "height and width must be at least 1 when batch is not 0"),
    (carve, dict(channels=-1), "channels is negative"), (carve, dict(channel=2), "channel out of range (0 .. channels - 1)"),
    (carve, dict(channel=-1), "channel out of range (0 .. channels - 1)"), (carve, dict(channels=0, channel=0), "channel out of range (0 .. channels - 1)"),
    (carve, dict(lo=1.0, hi=1.0), CUBE), (carve, dict(hi=nan), CUBE), (carve, dict(lo=-inf), CUBE), (carve, dict(lo=-1e308, hi=1e308), CUBE),
    (carve, dict(alpha=None), "alpha_dev" + NULL), (carve, dict(mvp=None), "mvp_dev" + NULL), (carve, dict(bits=None), "bits_workspace_dev" + NULL),
    (carve, dict(hull=None), "hull_out_dev" + NULL), (carve, dict(batch=0, alpha=None, mvp=None, bits=None, hull=None), "hull_out_dev" + NULL),
    (carve, dict(grid=0, batch=-1, lo=1.0, alpha=None), GRID1), (carve, dict(batch=-1, lo=1.0, alpha=None), IMAGE), (carve, dict(lo=1.0, alpha=None), CUBE),
    (carve, dict(mvp=None, hull=None), "mvp_dev" + NULL),
    (edt, dict(grid=0), GRID1), (edt, dict(grid=513), GRID1), (edt, dict(mask=None), "mask_dev" + NULL), (edt, dict(ws=None), "workspace_dev" + NULL),
    (edt, dict(d2=None), "d2_out_dev" + NULL), (edt, dict(status=None), "status_out_dev" + NULL), (edt, dict(grid=0, mask=None), GRID1), (edt, dict(ws=None, status=None), "workspace_dev" + NULL),
    (cover, dict(grid=0), GRID1), (cover, dict(grid=513), GRID1), (cover, dict(n=-1), "n_spheres out of range (0 .. 2^20)"), (cover, dict(n=(1 << 20) + 1), "n_spheres out of range (0 .. 2^20)"),
    (cover, dict(s2=-1.0), "s2, hs2 and m2 are squares: none may be negative or NaN"), (cover, dict(hs2=nan), "s2, hs2 and m2 are squares: none may be negative or NaN"),
    (cover, dict(hull=None), "hull_dev" + NULL), (cover, dict(d2=None), "d2_dev" + NULL), (cover, dict(ws=None), "workspace_dev" + NULL),
    (cover, dict(unc=None), "uncovered_out_dev" + NULL), (cover, dict(count=None), "count_out_dev" + NULL), (cover, dict(flat=None), "flat_out_dev" + NULL),
    (cover, dict(q=None), "q_out_dev" + NULL), (cover, dict(flat=None, count=None), "count_out_dev" + NULL),
    # ---- tsamd_union_field, _surface_count, _surface_emit (tests/test_merge.py) ----
    (field, dict(grid=1), GRID2), (field, dict(grid=513), GRID2), (field, dict(grid=-4), GRID2), (field, dict(nv=-1), NV_ELEM), (field, dict(nv=big), NV_ELEM),
    (field, dict(nt=-1), "n_tets out of range (0 .. 2^30)"), (field, dict(nt=(1 << 30) + 1), "n_tets out of range (0 .. 2^30)"), (field, dict(lo=1.0, hi=1.0), CUBE),
    (field, dict(lo=2.0), CUBE), (field, dict(hi=nan), CUBE), (field, dict(lo=-inf), CUBE), (field, dict(lo=-1e308, hi=1e308), CUBE), (field, dict(tet_v=None), "tet_v_dev" + NULL),
    (field, dict(elem=None), "elem_dev" + NULL), (field, dict(out=None), "field_out_dev" + NULL), (field, dict(nt=0, tet_v=None, elem=None, out=None), "field_out_dev" + NULL),
    (field, dict(grid=1, nv=-1, lo=2.0), GRID2), (field, dict(nv=-1, nt=-1, lo=2.0), NV_ELEM), (field, dict(nt=-1, lo=2.0, out=None), "n_tets out of range (0 .. 2^30)"),
    (field, dict(tet_v=None, elem=None), "elem_dev" + NULL),
    (count, dict(grid=1), GRID2), (count, dict(grid=513), GRID2), (count, dict(level=nan), LEVEL), (count, dict(f=None), "field_dev" + NULL),
    (count, dict(vmask=None), "vmask_out_dev" + NULL), (count, dict(vcount=None), "vcount_out_dev" + NULL), (count, dict(tcount=None), "tcount_out_dev" + NULL),
    (count, dict(flag=None), "open_out_dev" + NULL), (count, dict(grid=1, level=nan), GRID2), (count, dict(level=nan, f=None), LEVEL),
    (emit, dict(grid=1), GRID2), (emit, dict(grid=513), GRID2), (emit, dict(lo=1.0, hi=-1.0), CUBE), (emit, dict(level=nan), LEVEL), (emit, dict(lo=1.0, hi=-1.0, level=nan), CUBE),
    (emit, dict(nv=-1), "n_vertices out of range (0 .. 7 grid^3)"), (emit, dict(nt=-1), "n_triangles out of range (0 .. 12 grid^3)"),
    (emit, dict(nv=7 * 512 + 1), "n_vertices out of range (0 .. 7 grid^3)"), (emit, dict(nt=12 * 512 + 1), "n_triangles out of range (0 .. 12 grid^3)"),
    (emit, dict(f=None), "field_dev" + NULL), (emit, dict(vmask=None), "vmask_dev" + NULL), (emit, dict(voff=None), "voffset_dev" + NULL), (emit, dict(toff=None), "toffset_dev" + NULL),
    (emit, dict(v=None), "v_out_dev" + NULL), (emit, dict(faces=None), "faces_out_dev" + NULL), (emit, dict(nv=0, nt=0, f=None), "field_dev" + NULL),
    # ---- tsamd_grid_components, _field_fill (tests/test_merge_fill.py) ----
    (comps, dict(grid=1), GRID2), (comps, dict(grid=513), GRID2), (comps, dict(grid=-4), GRID2), (comps, dict(level=nan), LEVEL), (comps, dict(f=None), "field_dev" + NULL),
    (comps, dict(label=None), "label_out_dev" + NULL), (comps, dict(status=None), "status_out_dev" + NULL),
    (fill, dict(grid=1), GRID2), (fill, dict(grid=513), GRID2), (fill, dict(level=nan), LEVEL), (fill, dict(mode=0), "mode must be TSAMD_FILL_CAVITIES (1) or TSAMD_FILL_OUTER (2)"),
    (fill, dict(mode=3), "mode must be TSAMD_FILL_CAVITIES (1) or TSAMD_FILL_OUTER (2)"), (fill, dict(mode=-1), "mode must be TSAMD_FILL_CAVITIES (1) or TSAMD_FILL_OUTER (2)"),
    (fill, dict(level=nan, mode=0), LEVEL), (fill, dict(f=None), "field_dev" + NULL), (fill, dict(work=None), "workspace_dev" + NULL), (fill, dict(out=None), "field_out_dev" + NULL),
    (fill, dict(stats=None), "stats_out_dev" + NULL), (fill, dict(out=p), "field_out_dev must not be field_dev (the input is never modified)"), (fill, dict(work=half), "workspace_dev" + A8),
    (fill, dict(work=half, stats=None), "stats_out_dev" + NULL), (fill, dict(work=half, out=p), "field_out_dev must not be field_dev (the input is never modified)"),
    # ---- tsamd_nearest_points, _sample_surface, _nearest_points_info (tests/test_metrics.py) ----
    (near, dict(n=-1), "n out of range (0 .. 2^31 - 1)"), (near, dict(n=big), "n out of range (0 .. 2^31 - 1)"), (near, dict(m=0), "m out of range (1 .. 2^31 - 1: a query needs a ref point)"),
    (near, dict(m=-3), "m out of range (1 .. 2^31 - 1: a query needs a ref point)"), (near, dict(m=big), "m out of range (1 .. 2^31 - 1: a query needs a ref point)"),
    (near, dict(chunks=-1), "ref_chunks out of range (0 = automatic, else 1 .. min(m, 65535))"), (near, dict(chunks=5), "ref_chunks out of range (0 = automatic, else 1 .. min(m, 65535))"),
    (near, dict(m=70000, chunks=65536), "ref_chunks out of range (0 = automatic, else 1 .. min(m, 65535))"), (near, dict(q=None), "query_dev" + NULL), (near, dict(r=None), "ref_dev" + NULL),
    (near, dict(work=None), "workspace_dev" + NULL), (near, dict(d2=None), "d2_out_dev" + NULL), (near, dict(idx=None), "idx_out_dev" + NULL), (near, dict(q=odd), "query_dev" + A4),
    (near, dict(r=odd), "ref_dev" + A4), (near, dict(work=half), "workspace_dev" + A8), (near, dict(d2=odd), "d2_out_dev" + A4), (near, dict(idx=odd), "idx_out_dev" + A4),
    (near, dict(q=odd, idx=None), "idx_out_dev" + NULL), (near, dict(r=odd, idx=odd), "ref_dev" + A4),
    (weights, dict(phase=2), "phase must be TSAMD_SAMPLE_WEIGHTS (0) or TSAMD_SAMPLE_DRAW (1)"), (weights, dict(phase=-1), "phase must be TSAMD_SAMPLE_WEIGHTS (0) or TSAMD_SAMPLE_DRAW (1)"),
    (weights, dict(nv=-1), NV_FACES), (weights, dict(nv=big), NV_FACES), (weights, dict(nt=0), "n_triangles out of range (1 .. 2^31 - 1)"), (weights, dict(nt=big), "n_triangles out of range (1 .. 2^31 - 1)"),
    (weights, dict(v=None), "v_dev" + NULL), (weights, dict(f=None), "faces_dev" + NULL), (weights, dict(prefix=None), "prefix_dev" + NULL), (weights, dict(work=None), "workspace_dev" + NULL),
    (weights, dict(v=odd), "v_dev" + A4), (weights, dict(f=odd), "faces_dev" + A4), (weights, dict(prefix=half), "prefix_dev" + A8), (weights, dict(work=half), "workspace_dev" + A8),
    (weights, dict(f=odd, prefix=None), "prefix_dev" + NULL), (weights, dict(f=odd, v=None), "faces_dev" + A4), (weights, dict(v=odd, work=None), "v_dev" + A4),
    (draw, dict(n=-1), "n_samples out of range (0 .. 2^31 - 1)"), (draw, dict(n=big), "n_samples out of range (0 .. 2^31 - 1)"), (draw, dict(nt=0), "n_triangles out of range (1 .. 2^31 - 1)"),
    (draw, dict(v=None), "v_dev" + NULL), (draw, dict(f=None), "faces_dev" + NULL), (draw, dict(prefix=None), "prefix_dev" + NULL), (draw, dict(pts=None), "points_out_dev" + NULL),
    (draw, dict(nrm=None), "normals_out_dev" + NULL), (draw, dict(tri=None), "tri_out_dev" + NULL), (draw, dict(prefix=half), "prefix_dev" + A8), (draw, dict(pts=odd), "points_out_dev" + A4),
    (draw, dict(nrm=odd), "normals_out_dev" + A4), (draw, dict(tri=odd), "tri_out_dev" + A4), (draw, dict(pts=odd, tri=None), "tri_out_dev" + NULL),
    (info, dict(n=-1), "n out of range (0 .. 2^31 - 1)"), (info, dict(m=big), "m out of range (0 .. 2^31 - 1)"), (info, dict(out=(0, 1, 1, 1)), "block_out" + NULL),
    (info, dict(out=(1, 0, 1, 1)), "queries_per_lane_out" + NULL), (info, dict(out=(1, 1, 0, 1)), "ref_tile_out" + NULL), (info, dict(out=(1, 1, 1, 0)), "auto_chunks_out" + NULL),
    # ---- tsamd_simplify_keys, _cells, _faces, _dedupe (tests/test_simplify.py) ----
    (keys, dict(nv=-1), NV_FACES), (keys, dict(nv=big), NV_FACES), (keys, dict(nt=-1), NT_SIMPLIFY), (keys, dict(nt=(big - 1) // 3 + 1), NT_SIMPLIFY), (keys, dict(cells=0), "cells out of range (1 .. 1024)"),
    (keys, dict(cells=1025), "cells out of range (1 .. 1024)"), (keys, dict(lo=1.0), CUBE_CELLS), (keys, dict(hi=nan), CUBE_CELLS), (keys, dict(hi=inf), CUBE_CELLS),
    (keys, dict(lo=0.0, hi=5e-324), CUBE_CELLS), (keys, dict(lo=-1e308, hi=1e308), CUBE_CELLS), (keys, dict(nv=-1, cells=0), NV_FACES), (keys, dict(cells=0, lo=1.0), "cells out of range (1 .. 1024)"),
    (keys, dict(v=None), "v_dev" + NULL), (keys, dict(f=None), "faces_dev" + NULL), (keys, dict(vkey=None), "vkey_out_dev" + NULL), (keys, dict(rec=None), "records_out_dev" + NULL),
    (keys, dict(state=None), "state_out_dev" + NULL), (keys, dict(v=odd), "v_dev" + A4), (keys, dict(vkey=odd), "vkey_out_dev" + A4), (keys, dict(f=odd), "faces_dev" + A4),
    (keys, dict(rec=half), "records_out_dev" + A8), (keys, dict(v=odd, vkey=None), "vkey_out_dev" + NULL), (keys, dict(f=odd, state=None), "state_out_dev" + NULL),
    (keys, dict(v=odd, f=None), "v_dev" + A4),
    (cells_, dict(placement=2), "placement must be TSAMD_SIMPLIFY_QUADRIC (0) or TSAMD_SIMPLIFY_MEAN (1)"), (cells_, dict(stab=-1.0), "stabilise must be a finite number >= 0"),
    (cells_, dict(stab=nan), "stabilise must be a finite number >= 0"), (cells_, dict(cells=0), "cells out of range (1 .. 1024)"), (cells_, dict(nt=-1), NT_SIMPLIFY),
    (cells_, dict(status=None), "status_out_dev" + NULL), (cells_, dict(status=odd), "status_out_dev" + A4), (cells_, dict(vkey=None), "vkey_dev" + NULL), (cells_, dict(rec=None), "records_dev" + NULL),
    (cells_, dict(perm=None), "perm_dev" + NULL), (cells_, dict(pos=None), "pos_out_dev" + NULL), (cells_, dict(head=None), "head_out_dev" + NULL), (cells_, dict(run=None), "run_out_dev" + NULL),
    (cells_, dict(perm=half), "perm_dev" + A8), (cells_, dict(run=odd), "run_out_dev" + A4), (cells_, dict(f=odd, run=None), "run_out_dev" + NULL), (cells_, dict(status=odd, v=None), "status_out_dev" + A4),
    (cells_, dict(placement=2, stab=-1.0, status=None), "placement must be TSAMD_SIMPLIFY_QUADRIC (0) or TSAMD_SIMPLIFY_MEAN (1)"),
    (faces_, dict(nt=-1), NT_SIMPLIFY), (faces_, dict(run=None), "run_dev" + NULL), (faces_, dict(state=None), "state_dev" + NULL), (faces_, dict(tri=None), "tri_out_dev" + NULL),
    (faces_, dict(ab=None), "key_ab_out_dev" + NULL), (faces_, dict(c=None), "key_c_out_dev" + NULL), (faces_, dict(ab=half), "key_ab_out_dev" + A8), (faces_, dict(run=odd, c=None), "key_c_out_dev" + NULL),
    (dedupe, dict(nt=-1), NT_SIMPLIFY), (dedupe, dict(tri=None), "tri_dev" + NULL), (dedupe, dict(order=None), "order_dev" + NULL), (dedupe, dict(keep=None), "keep_out_dev" + NULL),
    (dedupe, dict(used=None), "used_out_dev" + NULL), (dedupe, dict(status=None), "status_out_dev" + NULL), (dedupe, dict(order=half), "order_dev" + A8),
    (dedupe, dict(tri=odd, used=None), "used_out_dev" + NULL), (dedupe, dict(status=odd, tri=None), "status_out_dev" + A4),
]
# ---- tsamd_voxel_winding, _occupancy (tests/test_voxelize.py): what the two share, then each one's own ----
C_CASES += [(fn, kw, msg) for fn in (wind, occ_) for kw, msg in [
    (dict(grid=0), GRID1), (dict(grid=513), GRID1), (dict(grid=-4), GRID1), (dict(nv=-1), NV_FACES), (dict(nv=1 << 31), NV_FACES), (dict(nt=-1), "n_triangles out of range (0 .. 2^31 - 1)"),
    (dict(nt=1 << 31), "n_triangles out of range (0 .. 2^31 - 1)"), (dict(lo=1.0, hi=1.0), CUBE_GRID), (dict(lo=2.0), CUBE_GRID), (dict(hi=nan), CUBE_GRID), (dict(lo=-inf), CUBE_GRID),
    (dict(lo=-1e308, hi=1e308), CUBE_GRID), (dict(lo=0.0, hi=5e-324), CUBE_GRID), (dict(nv=-1, nt=-1, grid=0), NV_FACES), (dict(nt=-1, grid=0, lo=2.0), "n_triangles out of range (0 .. 2^31 - 1)"),
    (dict(grid=0, lo=2.0, ws=None), GRID1), (dict(v=None), "v_dev" + NULL), (dict(faces=None), "faces_dev" + NULL), (dict(ws=None), "workspace_dev" + NULL), (dict(stats=None), "stats_out_dev" + NULL),
    (dict(stats=p + 4), "stats_out_dev" + A8), (dict(ws=p + 4), "workspace_dev" + A8), (dict(v=p + 1), "v_dev" + A4), (dict(faces=p + 2), "faces_dev" + A4),
    (dict(ws=p + 4, stats=None), "stats_out_dev" + NULL), (dict(faces=p + 2, v=None), "faces_dev" + A4), (dict(stats=p + 4, faces=None), "stats_out_dev" + A8)]]
C_CASES += [
    (wind, dict(axis=3), "axis must be 0, 1 or 2"), (wind, dict(axis=-1), "axis must be 0, 1 or 2"), (wind, dict(w=None), "w_out_dev" + NULL), (wind, dict(w=p + 2), "w_out_dev" + A4),
    (wind, dict(axis=3, w=None), "axis must be 0, 1 or 2"), (wind, dict(v=None, axis=3), "v_dev" + NULL),
    (occ_, dict(rule=3), "rule must be TSAMD_VOXEL_NONZERO (0), TSAMD_VOXEL_POSITIVE (1) or TSAMD_VOXEL_ODD (2)"),
    (occ_, dict(rule=-1), "rule must be TSAMD_VOXEL_NONZERO (0), TSAMD_VOXEL_POSITIVE (1) or TSAMD_VOXEL_ODD (2)"), (occ_, dict(rays=2), "rays must be 1 or 3"), (occ_, dict(rays=0), "rays must be 1 or 3"),
    (occ_, dict(rule=3, rays=2, out=None), "rule must be TSAMD_VOXEL_NONZERO (0), TSAMD_VOXEL_POSITIVE (1) or TSAMD_VOXEL_ODD (2)"), (occ_, dict(out=None), "occ_out_dev" + NULL),
    (wind, dict(nt=0, v=None, faces=None, w=None), "w_out_dev" + NULL), (occ_, dict(nt=0, v=None, faces=None, ws=None), "workspace_dev" + NULL),
]


def test_c_abi_messages_and_return_codes():
    lib = _lib()
    bad = []
    for fn, kw, want in C_CASES:
        rc = fn(**kw)
        got = lib.tsamd_last_error().decode()
        if rc != INVALID or got != want:
            bad.append((fn.__name__, kw, rc, got, want))
    assert bad == []
    # "nothing to write" returns before the pointers are looked at, and after the sizes
    assert emit(nv=0, nt=0, v=None, faces=None) == 0 and near(n=0, q=None, work=None, d2=None, idx=None) == 0
    assert draw(n=0, pts=None, nrm=None, tri=None) == 0 and faces_(nt=0, run=None, state=None, tri=None, ab=None, c=None) == 0
    assert near(n=0, m=0) == INVALID and draw(n=0, prefix=None) == INVALID and faces_(nt=-1, run=None) == INVALID
    assert lib.tsamd_voxel_workspace_bytes(0) == -1 and lib.tsamd_voxel_workspace_bytes(513) == -1 and lib.tsamd_nearest_points_workspace_bytes(big) == -1
    assert _capi.ABI_VERSION == 3 and lib.tsamd_abi_version() == 3
