"""ctypes binding of include/tssplat_amd.h (libtssplat_amd.so).

The library is the product; this file is plumbing.  There is deliberately no
Python/CPU fallback: if the shared library cannot be loaded, importing the
operator surface raises.
"""
from __future__ import annotations

import ctypes as C
import os

from . import _build

_lib = None


class TsamdError(RuntimeError):
    """A C-ABI call failed (the reference surfaces native failures as RuntimeError too,
    /root/reference/tssplat_ext/tet_spheres/cudaUtils.h:10-44)."""

    def __init__(self, code: int, message: str):
        super().__init__(f"tssplat_amd error {code}: {message}")
        self.code = code


class Options(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32),
        ("device", C.c_int32),
        ("lds_budget_bytes", C.c_int32),
        ("max_threads", C.c_int32),
        ("target_owned", C.c_int32),
        ("lane_search_sweeps", C.c_int32),
        ("host_only", C.c_int32),
        ("num_threads", C.c_int32),
        ("debug_flags", C.c_int32),
        ("slots_per_thread", C.c_int32),
        ("rebuild_dminv", C.c_int32),
        ("abi_version", C.c_int32),
    ]


class PlanInfo(C.Structure):
    _fields_ = [
        ("n_vertices", C.c_int64), ("n_tets", C.c_int64), ("n_tiles", C.c_int64),
        ("n_components", C.c_int64), ("total_slots", C.c_int64), ("total_tile_vertices", C.c_int64),
        ("shared_vertex_copies", C.c_int64), ("finish_vertices", C.c_int64), ("device_bytes", C.c_int64),
        ("max_slots", C.c_int32), ("max_tile_vertices", C.c_int32), ("block_threads", C.c_int32),
        ("lds_bytes", C.c_int32), ("slots_per_thread", C.c_int32), ("n_planes", C.c_int32),
    ]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class PartitionInfo(C.Structure):
    _fields_ = [
        ("owned_tets", C.c_int64), ("halo_slots", C.c_int64), ("staged_rows", C.c_int64), ("n_tiles", C.c_int64),
        ("tile_capacity", C.c_int64), ("min_tiles", C.c_int64), ("cut_components", C.c_int64),
        ("bisection_components", C.c_int64), ("cut_templates", C.c_int64), ("mean_fill", C.c_double), ("max_fill", C.c_double),
    ]


class TileView(C.Structure):
    _fields_ = [
        ("n_slots", C.c_int32), ("n_owned", C.c_int32), ("s_pad", C.c_int32), ("n_verts", C.c_int32),
        ("n_excl", C.c_int32), ("stage_off", C.c_int64), ("n_rows", C.c_int32), ("rec_base", C.c_int32),
        ("planes", C.POINTER(C.c_uint32)), ("row_start", C.POINTER(C.c_uint16)),
        ("gvid", C.POINTER(C.c_int32)), ("vdst", C.POINTER(C.c_int32)), ("slot_tet", C.POINTER(C.c_int32)), ("rest", C.POINTER(C.c_float)),
    ]


class BlendPlanStruct(C.Structure):
    """``tsamd_blend_plan``: device pointers and sizes of a blend plan (tssplat_amd/dr.py: BlendPlan)."""
    _fields_ = [
        ("struct_size", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("reserved", C.c_int32),
        ("batch", C.c_int64), ("n_points", C.c_int64), ("n_blends", C.c_int64), ("n_dst", C.c_int64), ("n_src", C.c_int64),
        ("pix_point_dev", C.c_void_p), ("pix_dst_dev", C.c_void_p),
        ("dst_ptr_dev", C.c_void_p), ("dst_src_pix_dev", C.c_void_p), ("dst_src_point_dev", C.c_void_p), ("dst_weight_dev", C.c_void_p),
        ("src_ptr_dev", C.c_void_p), ("src_dst_pix_dev", C.c_void_p), ("src_dst_slot_dev", C.c_void_p), ("src_weight_dev", C.c_void_p),
        ("point_pix_dev", C.c_void_p), ("point_dst_dev", C.c_void_p), ("point_src_dev", C.c_void_p),
    ]


class SmoothMeshStruct(C.Structure):
    """``tsamd_smooth_mesh``: sizes and device pointers of a vertex adjacency (tssplat_amd/smooth.py: VertexAdjacency)."""
    _fields_ = [
        ("struct_size", C.c_int32), ("reserved", C.c_int32),
        ("n_vertices", C.c_int64), ("n_triangles", C.c_int64), ("n_neighbours", C.c_int64), ("n_face_entries", C.c_int64),
        ("offsets_dev", C.c_void_p), ("neighbours_dev", C.c_void_p),
        ("face_offsets_dev", C.c_void_p), ("faces_of_dev", C.c_void_p), ("faces_dev", C.c_void_p),
    ]


ABI_VERSION = 3          # include/tssplat_amd.h: TSAMD_ABI_VERSION

# every symbol include/tssplat_amd.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "tsamd_last_error": (C.c_char_p, []),
    "tsamd_version": (C.c_char_p, []),
    "tsamd_abi_version": (C.c_int32, []),
    "tsamd_create": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(Options), C.POINTER(C.c_void_p)]),
    "tsamd_create_with_operator": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.POINTER(Options), C.POINTER(C.c_void_p)]),
    "tsamd_create_from_veg": (C.c_int, [C.c_char_p, C.POINTER(Options), C.POINTER(C.c_void_p)]),
    "tsamd_destroy": (None, [C.c_void_p]),
    "tsamd_num_vertices": (C.c_int64, [C.c_void_p]),
    "tsamd_num_tets": (C.c_int64, [C.c_void_p]),
    "tsamd_get_plan_info": (C.c_int, [C.c_void_p, C.POINTER(PlanInfo)]),
    "tsamd_get_partition_info": (C.c_int, [C.c_void_p, C.POINTER(PartitionInfo)]),
    "tsamd_get_tile": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(TileView)]),
    "tsamd_get_finish_lists": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.POINTER(C.c_int32)),
                                         C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.POINTER(C.c_int32))]),
    "tsamd_get_index_reps": (C.c_int, [C.c_void_p, C.POINTER(C.POINTER(C.c_int32))]),
    "tsamd_get_regular_batch": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "tsamd_get_adjacency": (C.c_int, [C.c_void_p, C.POINTER(C.POINTER(C.c_int32))]),
    "tsamd_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p]),
    "tsamd_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_void_p,
                                 C.c_void_p]),
    "tsamd_forward_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_int,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsamd_evaluate_dev_coef": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "tsamd_graph_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "tsamd_graph_launch": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_void_p]),
    "tsamd_graph_launch_to": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsamd_graph_destroy": (None, [C.c_void_p]),
    "tsamd_read_energy_terms": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    "tsamd_set_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "tsamd_get_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "tsamd_scale": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "tsamd_adam_uniform_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_float,
                                        C.c_float, C.c_int64, C.c_float, C.c_void_p, C.c_void_p]),
    "tsamd_grad_limit_workspace_bytes": (C.c_int64, []),
    "tsamd_grad_limit": (C.c_int, [C.c_void_p, C.c_int64, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "tsamd_train_loop_workspace_bytes": (C.c_int64, [C.c_int32]),
    "tsamd_train_loop_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                          C.POINTER(C.c_void_p)]),
    "tsamd_train_loop_launch": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_float, C.c_float,
                                          C.c_float, C.c_int64, C.POINTER(C.c_float), C.c_void_p]),
    "tsamd_train_loop_destroy": (None, [C.c_void_p]),
    # renderer slice
    "tsamd_rasterize_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int64, C.c_int32, C.c_int32]),
    "tsamd_pair_masks_bytes": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    "tsamd_rasterize": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p]),
    "tsamd_interpolate": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                    C.c_void_p, C.c_void_p]),
    "tsamd_interpolate_backward": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32,
                                             C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsamd_rasterize_backward": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p]),
    "tsamd_antialias_topology_workspace_bytes": (C.c_int64, [C.c_int64]),
    "tsamd_antialias_topology": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsamd_antialias_prepared_bytes": (C.c_int64, [C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32]),
    "tsamd_antialias_prepare": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32,
                                          C.c_int32, C.c_void_p, C.c_void_p]),
    "tsamd_antialias": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32,
                                  C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "tsamd_antialias_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                           C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsamd_silhouette": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsamd_silhouette_backward": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    "tsamd_silhouette_mse_workspace_bytes": (C.c_int64, [C.c_int64]),
    "tsamd_silhouette_mse": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsamd_silhouette_mse_backward": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]),
    # the depth term from the alpha stage's ids
    "tsamd_depth_mse_workspace_bytes": (C.c_int64, [C.c_int64]),
    "tsamd_depth_mse": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsamd_depth_mse_backward": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    # the normal term (any [V, 3] vertex attribute) from the alpha stage's ids
    "tsamd_normal_mse_workspace_bytes": (C.c_int64, [C.c_int64]),
    "tsamd_normal_mse": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsamd_normal_mse_backward": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    # the texture stage's image side under a blend plan
    "tsamd_shade_plan_count": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                         C.c_void_p, C.c_void_p]),
    "tsamd_shade_plan_fill": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                        C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsamd_shade": (C.c_int, [C.POINTER(BlendPlanStruct), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsamd_shade_backward": (C.c_int, [C.POINTER(BlendPlanStruct), C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsamd_shade_l1_workspace_bytes": (C.c_int64, [C.c_int64]),
    "tsamd_shade_l1": (C.c_int, [C.POINTER(BlendPlanStruct), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsamd_shade_l1_backward": (C.c_int, [C.POINTER(BlendPlanStruct), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # surface glue
    "tsamd_extract_surface": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p,
                                      C.POINTER(C.c_int64)]),
    "tsamd_surface_create": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.POINTER(C.c_void_p)]),
    "tsamd_surface_destroy": (None, [C.c_void_p]),
    "tsamd_surface_positions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsamd_surface_positions_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsamd_vertex_normals": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsamd_vertex_normals_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # hash-grid encoding (the texture stage's colour field)
    "tsamd_grid_layout": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.POINTER(C.c_int64)]),
    "tsamd_grid_encode": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32,
                                    C.c_void_p, C.c_void_p]),
    "tsamd_grid_encode_backward": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                             C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsamd_grid_sorted_chunk_points": (C.c_int64, []),
    "tsamd_grid_backward_sorted_workspace_bytes": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32,
                                                             C.POINTER(C.c_int64)]),
    "tsamd_grid_encode_backward_sorted": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float,
                                                    C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "tsamd_grid_plan_bytes": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.POINTER(C.c_int64)]),
    "tsamd_grid_plan_build": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_void_p,
                                        C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "tsamd_grid_backward_planned_workspace_bytes": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32,
                                                              C.POINTER(C.c_int64)]),
    "tsamd_grid_encode_backward_planned": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    # fully fused MLP (the colour MLP of a tcnn network config)
    "tsamd_mlp_layout": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64),
                                   C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "tsamd_mlp_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "tsamd_mlp_forward": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                    C.c_void_p, C.c_void_p]),
    "tsamd_mlp_backward": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # texture atlas and texture sampling (the texture stage's export)
    "tsamd_atlas_layout": (C.c_int, [C.c_int64, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "tsamd_atlas_bake_positions": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsamd_texture": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                C.c_int32, C.c_void_p, C.c_void_p]),
    "tsamd_texture_backward": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                         C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # sphere initialisation: visual hull, squared distance transform, greedy ball cover
    "tsamd_hull_carve": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_int32, C.c_double,
                                   C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsamd_edt_squared": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsamd_greedy_cover": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # merging tet-spheres: union field on the voxel grid, marching tetrahedra in a count and an emit phase
    "tsamd_union_field": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_double, C.c_double, C.c_void_p, C.c_void_p]),
    "tsamd_surface_count": (C.c_int, [C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsamd_surface_emit": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    # the merge's flood fill: connected components of the field's nodes, cavities filled, islands dropped
    "tsamd_grid_components": (C.c_int, [C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsamd_field_fill": (C.c_int, [C.c_void_p, C.c_int32, C.c_float, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # surface metrics: area-uniform surface samples (weights; draw) and the all-pairs nearest-point search
    "tsamd_sample_surface": (C.c_int, [C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsamd_nearest_points_workspace_bytes": (C.c_int64, [C.c_int64]),
    "tsamd_nearest_points_info": (C.c_int, [C.c_int64, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "tsamd_nearest_points": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # the exact point-to-triangle search: closest triangle, squared distance and closest point per query
    "tsamd_nearest_on_mesh_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int64]),
    "tsamd_nearest_on_mesh_info": (C.c_int, [C.c_int64, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "tsamd_nearest_on_mesh": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    # surface simplification: cell keys and record slots, the per-cell run walk and solve, the face triples, the duplicate flags
    "tsamd_simplify_keys": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "tsamd_simplify_cells": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_double, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsamd_simplify_faces": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsamd_simplify_dedupe": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # voxelising triangle meshes: the integer winding number on the merge's grid, and the occupancy made of it
    "tsamd_voxel_workspace_bytes": (C.c_int64, [C.c_int32]),
    "tsamd_voxel_winding": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    "tsamd_voxel_occupancy": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    # mesh quality: lattice snap and per-triangle record, the crossing-pair search, edge keys, fan pairs, union-find
    "tsamd_quality_info": (C.c_int, [C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "tsamd_quality_prepare": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "tsamd_quality_pairs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsamd_quality_edges": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsamd_quality_fan_pairs": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsamd_quality_union": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]),
    # surface smoothing: directed edge keys and vertex-face keys, the rows of the adjacency, who moves, one half-step, a whole run
    "tsamd_smooth_keys": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsamd_smooth_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsamd_smooth_classify": (C.c_int, [C.c_void_p, C.POINTER(SmoothMeshStruct), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "tsamd_smooth_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(SmoothMeshStruct), C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_double,
                                    C.c_void_p]),
    "tsamd_smooth_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(SmoothMeshStruct), C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_int32,
                                   C.c_void_p, C.c_double, C.POINTER(C.c_int32), C.c_void_p]),
}


def lib_path() -> str:
    return _build.LIB


def load(build_if_missing: bool = True):
    """Load libtssplat_amd.so (building it in-tree first if hipcc is around and it is stale/missing)."""
    global _lib
    if _lib is not None:
        return _lib
    # The host framework's HIP runtime must be in the process first: torch bundles its own
    # libamdhip64.so.7, and a second copy (from /opt/rocm) loaded ahead of it leaves one of the
    # two runtimes without devices ("no HIP device is visible").
    import torch  # noqa: F401
    path = _build.LIB
    override = os.environ.get("TSSPLAT_AMD_LIB")       # experiment builds (tssplat_amd._build.build_variant)
    if override:
        path, build_if_missing = override, False
    if build_if_missing:
        try:
            path = _build.build()
        except Exception:
            if not os.path.exists(path):
                raise
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build it with `python -m tssplat_amd._build` (needs hipcc, --offload-arch=gfx950). "
            "tssplat_amd has no CPU fallback.")
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)       # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    if lib.tsamd_abi_version() != ABI_VERSION:
        raise ImportError(f"{path}: ABI version {lib.tsamd_abi_version()}, these bindings are written for {ABI_VERSION} "
                          "(include/tssplat_amd.h: TSAMD_ABI_VERSION) -- rebuild the library")
    _lib = lib
    return lib


_ext_module = None


def autograd_ext(build_if_missing: bool = True):
    """The C++ torch extension (csrc/torch_autograd.cpp + csrc/torch_exchange.cpp, tssplat_amd/_tsamd_autograd.so): the autograd
    nodes of the energy and the energy exchange's helper thread, wired to the entry points of the library loaded above.  Like
    :func:`load` there is no fallback: if the extension cannot be built or imported, this raises."""
    global _ext_module
    if _ext_module is not None:
        return _ext_module
    lib = load()
    if build_if_missing:
        try:
            _build.build_torch_ext()
        except Exception:
            if not os.path.exists(_build.TORCH_EXT):
                raise
    if not os.path.exists(_build.TORCH_EXT):
        raise ImportError(
            f"{_build.TORCH_EXT} is missing: build it with `python -m tssplat_amd._build` (needs g++ and the torch headers). "
            "tssplat_amd has no Python fallback for it.")
    import importlib
    ext = importlib.import_module("tssplat_amd._tsamd_autograd")
    addr = lambda fn: C.cast(fn, C.c_void_p).value
    ext.set_entry_points(addr(lib.tsamd_graph_launch), addr(lib.tsamd_forward_backward), addr(lib.tsamd_last_error))
    _ext_module = ext
    return ext


def check(rc: int) -> None:
    if rc != 0:
        raise TsamdError(rc, load().tsamd_last_error().decode("utf-8", "replace"))


def make_options(**kw) -> Options:
    o = Options()
    o.struct_size = C.sizeof(Options)
    o.abi_version = ABI_VERSION
    o.device = -1
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError(f"unknown tsamd option {k!r}")
        setattr(o, k, int(v))
    return o
