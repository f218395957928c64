"""ctypes loader of the C-ABI shared library ``libfiesta_hip.so`` (see include/fiesta_hip.h).

There is deliberately no fallback: if the HIP library is missing or no gfx950 device is usable the
product path fails loudly (``FiestaHipError``).  Nothing under ``oracle/`` is ever imported here.
"""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfiesta_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "fiesta_hip.h")


class FiestaHipError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"fiesta_hip error {code}: {message}")
        self.code = code


class Config(C.Structure):
    _fields_ = [("mode", C.c_int32), ("device", C.c_int32), ("origin", C.c_double * 3),
                ("resolution", C.c_double), ("map_size", C.c_double * 3), ("reserve_size", C.c_int32),
                ("update_engine", C.c_int32), ("shard_lo", C.c_int32 * 3), ("global_grid", C.c_int32 * 3)]


class Stats(C.Structure):
    _fields_ = [("inserted", C.c_int64), ("deleted", C.c_int64), ("invalidated", C.c_int64),
                ("rounds", C.c_int64), ("tile_visits", C.c_int64), ("sweeps", C.c_int64),
                ("voxel_writes", C.c_int64), ("device_ms", C.c_double), ("host_ms", C.c_double),
                ("relax_ms", C.c_double), ("relax_launches", C.c_int64), ("prof", C.c_int64 * 8),
                ("bulk", C.c_int64), ("ft_rows_ms", C.c_double), ("ft_plane_ms", C.c_double), ("ft_x_ms", C.c_double),
                ("ft_overflow", C.c_int64 * 6), ("observed_voxels", C.c_int64), ("occupied_voxels", C.c_int64),
                ("ft_max_d2", C.c_int64), ("dropped_observations", C.c_int64), ("levels", C.c_int64), ("grid_levels", C.c_int64),
                ("cells", C.c_int64), ("nn_cells_ms", C.c_double), ("nn_lists_ms", C.c_double), ("nn_fill_ms", C.c_double),
                ("nn_entries", C.c_int64), ("nn_failed", C.c_int64),
                ("nn_incremental", C.c_int64), ("nn_dirty_cells", C.c_int64), ("nn_brute_cells", C.c_int64), ("masked", C.c_int64), ("mask_uncertified", C.c_int64), ("mask_iterations", C.c_int64), ("mask_walks", C.c_int64), ("mask_quads", C.c_int64),
                ("mask_certify_ms", C.c_double), ("mask_repair_ms", C.c_double), ("path_notes", C.c_int64)]

    # fiesta_hip_stats.path_notes (include/fiesta_hip.h: FIESTA_HIP_NOTE_*): why an update took the path it took
    NOTES = ("partly_observed", "partial_window", "window_history", "late_observation", "first_wave_pending", "density",
             "cells_backoff", "cells_failed", "incremental_redone", "small_delta", "masked_gave_up", "levels_gave_up", "sharded",
             "id_wrap", "engine_pinned")

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["prof"] = list(self.prof)
        d["ft_overflow"] = list(self.ft_overflow)
        d["why"] = [name for bit, name in enumerate(self.NOTES) if (self.path_notes >> bit) & 1]
        return d


class ShardInfo(C.Structure):
    _fields_ = [("local_dims", C.c_int32 * 3), ("local_origin", C.c_int32 * 3), ("owned_lo", C.c_int32 * 3),
                ("owned_hi", C.c_int32 * 3), ("global_grid", C.c_int32 * 3)]


class DepthFilter(C.Structure):
    _fields_ = [("tolerance", C.c_double), ("max_dist", C.c_double), ("min_dist", C.c_double), ("margin", C.c_int32),
                ("reset", C.c_int32), ("rel_transform", C.c_double * 16)]


class RaycastParams(C.Structure):
    _fields_ = [("min_ray_length", C.c_double), ("max_ray_length", C.c_double), ("l_cornor", C.c_double * 3),
                ("r_cornor", C.c_double * 3), ("dedup", C.c_int32), ("inverse", C.c_int32)]


class PathResult(C.Structure):
    """fiesta_hip_path_result: one array per output of fiesta_hip_path_clearance, every pointer nullable"""
    _fields_ = [("min_dist", C.c_void_p), ("min_index", C.c_void_p), ("min_pos", C.c_void_p), ("min_grad", C.c_void_p),
                ("first_below", C.c_void_p), ("first_below_pos", C.c_void_p), ("n_samples", C.c_void_p)]


class PathCostResult(C.Structure):
    """fiesta_hip_path_cost_result: one array per output of fiesta_hip_path_cost, every pointer nullable"""
    _fields_ = [("cost", C.c_void_p), ("grad", C.c_void_p), ("length", C.c_void_p), ("n_below", C.c_void_p),
                ("n_samples", C.c_void_p)]


class BodyResult(C.Structure):
    """fiesta_hip_body_result: one array per output of fiesta_hip_body_query, every pointer nullable"""
    _fields_ = [("min_clearance", C.c_void_p), ("min_sphere", C.c_void_p), ("min_pos", C.c_void_p), ("min_grad", C.c_void_p),
                ("n_below", C.c_void_p), ("cost", C.c_void_p), ("grad", C.c_void_p), ("sphere_clearance", C.c_void_p)]


class ArticulatedResult(C.Structure):
    """fiesta_hip_articulated_result: one array per output of fiesta_hip_articulated_query, every pointer nullable"""
    _fields_ = [("min_clearance", C.c_void_p), ("min_sphere", C.c_void_p), ("min_pos", C.c_void_p), ("min_grad", C.c_void_p),
                ("n_below", C.c_void_p), ("cost", C.c_void_p), ("frame_clearance", C.c_void_p), ("frame_cost", C.c_void_p),
                ("frame_grad", C.c_void_p), ("sphere_clearance", C.c_void_p)]


class SweepResult(C.Structure):
    """fiesta_hip_sweep_result: one array per output of fiesta_hip_body_sweep, every pointer nullable"""
    _fields_ = [("min_clearance", C.c_void_p), ("min_sample", C.c_void_p), ("min_sphere", C.c_void_p), ("min_pose", C.c_void_p),
                ("min_pos", C.c_void_p), ("min_grad", C.c_void_p), ("first_below", C.c_void_p), ("first_below_sphere", C.c_void_p),
                ("first_below_pose", C.c_void_p), ("n_below", C.c_void_p), ("n_samples", C.c_void_p)]


class RayResult(C.Structure):
    """fiesta_hip_ray_result: one array per output of fiesta_hip_ray_query, every pointer nullable"""
    _fields_ = [("n_visited", C.c_void_p), ("hit_index", C.c_void_p), ("hit_class", C.c_void_p), ("hit_vox", C.c_void_p),
                ("hit_dist", C.c_void_p), ("counts", C.c_void_p)]


class SkeletonResult(C.Structure):
    """fiesta_hip_skeleton_result: one array per output of fiesta_hip_get_skeleton_voxels, every pointer nullable"""
    _fields_ = [("vox", C.c_void_p), ("mask", C.c_void_p), ("d2", C.c_void_p), ("sep2", C.c_void_p)]


class ReachResult(C.Structure):
    """fiesta_hip_reach_result: one array per output of fiesta_hip_reach_field, every pointer nullable"""
    _fields_ = [("cost", C.c_void_p), ("target_cost", C.c_void_p)]


class ReachInfo(C.Structure):
    """fiesta_hip_reach_info: the clipped box and the counters of one fiesta_hip_reach_field call"""
    _fields_ = [("box_lo", C.c_int32 * 3), ("box_hi", C.c_int32 * 3), ("n_traversable", C.c_int64), ("n_seeds_used", C.c_int64),
                ("n_reached", C.c_int64), ("max_cost", C.c_int64), ("rounds", C.c_int64), ("tile_visits", C.c_int64)]


class ReachMatrixResult(C.Structure):
    """fiesta_hip_reach_matrix_result: one array per output of fiesta_hip_reach_matrix, every pointer nullable"""
    _fields_ = [("cost", C.c_void_p), ("source_status", C.c_void_p), ("source_reached", C.c_void_p)]


class ReachMatrixInfo(C.Structure):
    """fiesta_hip_reach_matrix_info: the clipped box and the counters of one fiesta_hip_reach_matrix call"""
    _fields_ = [("box_lo", C.c_int32 * 3), ("box_hi", C.c_int32 * 3), ("n_traversable", C.c_int64), ("n_sources_used", C.c_int64),
                ("fields", C.c_int64), ("batches", C.c_int64), ("rounds", C.c_int64), ("tile_visits", C.c_int64)]


class TourResult(C.Structure):
    """fiesta_hip_tour_result: one array per output of fiesta_hip_site_tour, every pointer nullable"""
    _fields_ = [("order", C.c_void_p), ("site_status", C.c_void_p), ("leg_cost", C.c_void_p), ("restart_length", C.c_void_p)]


class TourInfo(C.Structure):
    """fiesta_hip_tour_info: what one fiesta_hip_site_tour call found"""
    _fields_ = [("n_visited", C.c_int32), ("best_restart", C.c_int32), ("length", C.c_int64), ("nn_length", C.c_int64), ("moves", C.c_int64),
                ("capped", C.c_int64)]


class ReachPathsResult(C.Structure):
    """fiesta_hip_reach_paths_result: offsets is required, every other pointer nullable"""
    _fields_ = [("offsets", C.c_void_p), ("waypoints_vox", C.c_void_p), ("waypoints_pos", C.c_void_p), ("status", C.c_void_p),
                ("n_moves", C.c_void_p)]


class LegPathsResult(C.Structure):
    """fiesta_hip_leg_paths_result: offsets is required, every other pointer nullable"""
    _fields_ = [("offsets", C.c_void_p), ("waypoints_vox", C.c_void_p), ("waypoints_pos", C.c_void_p), ("status", C.c_void_p),
                ("n_moves", C.c_void_p), ("cost", C.c_void_p)]


class LegPathsInfo(C.Structure):
    """fiesta_hip_leg_paths_info: the batch a map retains from its last fiesta_hip_reach_matrix call"""
    _fields_ = [("box_lo", C.c_int32 * 3), ("box_hi", C.c_int32 * 3), ("connectivity", C.c_int32), ("reserved", C.c_int32),
                ("n_sources", C.c_int64)]


class FreeBoxesResult(C.Structure):
    """fiesta_hip_free_boxes_result: one array per output of fiesta_hip_free_boxes, every pointer nullable"""
    _fields_ = [("box", C.c_void_p), ("box_pos", C.c_void_p), ("stop", C.c_void_p), ("volume", C.c_void_p), ("status", C.c_void_p)]


class CorridorResult(C.Structure):
    """fiesta_hip_corridor_result: offsets is required, every other pointer nullable"""
    _fields_ = [("offsets", C.c_void_p), ("boxes", C.c_void_p), ("boxes_pos", C.c_void_p), ("stop", C.c_void_p), ("entry", C.c_void_p),
                ("status", C.c_void_p), ("n_chain", C.c_void_p), ("blocked_segment", C.c_void_p), ("blocked_vox", C.c_void_p)]


class RefineParams(C.Structure):
    """fiesta_hip_refine_params: the weights, step limits and iteration count of fiesta_hip_path_refine"""
    _fields_ = [("margin", C.c_double), ("w_obstacle", C.c_double), ("w_smooth", C.c_double), ("alpha", C.c_double),
                ("max_step", C.c_double), ("tolerance", C.c_double), ("iterations", C.c_int32), ("flags", C.c_int32)]


class RefineResult(C.Structure):
    """fiesta_hip_refine_result: one array per output of fiesta_hip_path_refine, every pointer nullable"""
    _fields_ = [("waypoints", C.c_void_p), ("cost", C.c_void_p), ("last_move", C.c_void_p), ("iterations", C.c_void_p),
                ("n_below", C.c_void_p), ("min_dist", C.c_void_p), ("status", C.c_void_p)]


class TimingParams(C.Structure):
    """fiesta_hip_timing_params: the sample spacing, the margin and the robot's speed and acceleration limits of fiesta_hip_path_timing"""
    _fields_ = [("step", C.c_double), ("margin", C.c_double), ("v_max", C.c_double), ("v_min", C.c_double), ("a_max", C.c_double),
                ("corner_dev", C.c_double), ("v_start", C.c_double), ("v_end", C.c_double)]


class TimingResult(C.Structure):
    """fiesta_hip_path_timing_result: one array per output of fiesta_hip_path_timing, every pointer nullable"""
    _fields_ = [("duration", C.c_void_p), ("length", C.c_void_p), ("n_samples", C.c_void_p), ("n_below", C.c_void_p),
                ("min_speed", C.c_void_p), ("min_index", C.c_void_p), ("status", C.c_void_p), ("time", C.c_void_p), ("speed", C.c_void_p)]


class BoundsResult(C.Structure):
    """fiesta_hip_bounds_result: one array per output of fiesta_hip_corridor_bounds, every pointer nullable"""
    _fields_ = [("bounds", C.c_void_p), ("ok", C.c_void_p), ("box", C.c_void_p)]


class ClusterResult(C.Structure):
    """fiesta_hip_cluster_result: one array per output of fiesta_hip_cluster_voxels, every pointer nullable"""
    _fields_ = [("label", C.c_void_p), ("size", C.c_void_p), ("root", C.c_void_p), ("box_lo", C.c_void_p), ("box_hi", C.c_void_p),
                ("centroid", C.c_void_p), ("mask_or", C.c_void_p), ("key_min", C.c_void_p), ("key_argmin", C.c_void_p),
                ("offsets", C.c_void_p), ("members", C.c_void_p)]


class ClusterInfo(C.Structure):
    """fiesta_hip_cluster_info: the totals of one fiesta_hip_cluster_voxels call, whatever the capacities"""
    _fields_ = [("n_clusters", C.c_int64), ("n_members", C.c_int64), ("n_invalid", C.c_int64), ("n_duplicates", C.c_int64),
                ("n_dropped_clusters", C.c_int64), ("largest", C.c_int64)]


class SplitResult(C.Structure):
    """fiesta_hip_split_result: one array per output of fiesta_hip_split_clusters, every pointer nullable"""
    _fields_ = [("parent", C.c_void_p), ("depth", C.c_void_p), ("size", C.c_void_p), ("root", C.c_void_p), ("box_lo", C.c_void_p),
                ("box_hi", C.c_void_p), ("centroid", C.c_void_p), ("mask_or", C.c_void_p), ("key_min", C.c_void_p), ("key_argmin", C.c_void_p),
                ("offsets", C.c_void_p), ("members", C.c_void_p), ("label", C.c_void_p)]


class SplitInfo(C.Structure):
    """fiesta_hip_split_info: the totals of one fiesta_hip_split_clusters call, whatever the capacity"""
    _fields_ = [("n_parts", C.c_int64), ("n_members", C.c_int64), ("n_split_clusters", C.c_int64), ("n_oversize", C.c_int64),
                ("largest", C.c_int64), ("depth", C.c_int64), ("status", C.c_int64)]


class ViewSet(C.Structure):
    """fiesta_hip_view_set: the candidate views of fiesta_hip_view_coverage, explicit (pos, dir, group, n_views) or ring (centroid, ring, n_ring)"""
    _fields_ = [("pos", C.c_void_p), ("dir", C.c_void_p), ("group", C.c_void_p), ("n_views", C.c_int64), ("centroid", C.c_void_p),
                ("ring", C.c_void_p), ("n_ring", C.c_int64)]


class ViewSensor(C.Structure):
    """fiesta_hip_view_sensor"""
    _fields_ = [("min_range", C.c_double), ("max_range", C.c_double), ("tan_h", C.c_double), ("tan_v", C.c_double),
                ("min_clearance", C.c_double), ("block_mask", C.c_int32), ("flags", C.c_int32), ("min_visible", C.c_int32),
                ("reserved", C.c_int32)]


class ViewResult(C.Structure):
    """fiesta_hip_view_result: one array per output of fiesta_hip_view_coverage, every pointer nullable"""
    _fields_ = [("view_class", C.c_void_p), ("n_in_view", C.c_void_p), ("n_visible", C.c_void_p), ("cover_count", C.c_void_p),
                ("first_view", C.c_void_p), ("best_view", C.c_void_p), ("best_count", C.c_void_p)]


class ViewInfo(C.Structure):
    """fiesta_hip_view_info: the totals of one fiesta_hip_view_coverage call"""
    _fields_ = [("n_usable", C.c_int64), ("n_pairs", C.c_int64), ("n_in_view", C.c_int64), ("n_visible", C.c_int64)]


def declared_symbols(header_path: str = HEADER_PATH):
    """Names of every function include/fiesta_hip.h declares (used by the CPU export test)."""
    text = open(header_path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fiesta_hip_[a-z0-9_]+)\s*\(", text)))


_lib = None


def _share_hip_runtime_with_torch():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so.7 (+ HSA runtime); libfiesta_hip.so needs the same
    SONAME from /opt/rocm.  Two HIP runtimes cannot share a process ("No HIP GPUs are available" in whichever
    initialises second), and which one wins would otherwise depend on import order.  If torch is installed, bind
    to its copy -- torch is only plumbing here (device buffers for the RCCL transport, bench.py), but it must be
    able to coexist.  Without torch the system ROCm runtime is used."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return  # torch's runtime is already mapped; the dynamic loader will reuse it by SONAME
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load():
    """Load libfiesta_hip.so (raises FiestaHipError if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FiestaHipError(-1, f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                 "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    _share_hip_runtime_with_torch()
    lib = C.CDLL(LIB_PATH)
    vp, i64, i32, dbl = C.c_void_p, C.c_int64, C.c_int32, C.c_double
    sig = {
        "fiesta_hip_last_error": (C.c_char_p, []),
        "fiesta_hip_version": (C.c_int, []),
        "fiesta_hip_device_count": (C.c_int, []),
        "fiesta_hip_create": (C.c_int, [vp, vp]),
        "fiesta_hip_destroy": (C.c_int, [vp]),
        "fiesta_hip_grid_size": (C.c_int, [vp, vp]),
        "fiesta_hip_grid_total_size": (C.c_int, [vp, vp]),
        "fiesta_hip_voxel_key": (C.c_int, [vp, vp, C.c_int64, vp]),
        "fiesta_hip_save": (C.c_int, [vp, C.c_char_p]),
        "fiesta_hip_load": (C.c_int, [vp, C.c_char_p]),
        "fiesta_hip_get_point_cloud": (C.c_int, [vp, i32, i32, vp, i64, vp]),
        "fiesta_hip_get_slice_marker": (C.c_int, [vp, i32, dbl, vp, vp, i64, vp]),
        "fiesta_hip_hash_window": (C.c_int, [vp, vp, vp]),
        "fiesta_hip_hash_recentre": (C.c_int, [vp, vp]),
        "fiesta_hip_rccl_unique_id": (C.c_int, [vp]),
        "fiesta_hip_shard_box": (C.c_int, [vp, C.c_int32, C.c_int32, vp, vp]),
        "fiesta_hip_shard_group_create": (C.c_int, [vp, vp, C.c_int32, C.c_int32, vp, vp]),
        "fiesta_hip_shard_group_create_hosted": (C.c_int, [vp, C.c_int32, C.c_int32, vp, vp]),
        "fiesta_hip_shard_group_precheck": (C.c_int, [vp, vp, C.c_int32, C.c_int32, C.c_int32]),
        "fiesta_hip_shard_group_comm_info": (C.c_int, [vp, vp, vp]),
        "fiesta_hip_shard_group_destroy": (C.c_int, [vp]),
        "fiesta_hip_shard_group_update_occupancy": (C.c_int, [vp, C.c_int32, vp, vp, vp]),
        "fiesta_hip_shard_group_update_esdf": (C.c_int, [vp, vp, vp, vp]),
        "fiesta_hip_set_prob_params": (C.c_int, [vp, dbl, dbl, dbl, dbl, dbl]),
        "fiesta_hip_set_update_range": (C.c_int, [vp, vp, vp, C.c_int]),
        "fiesta_hip_set_original_range": (C.c_int, [vp]),
        "fiesta_hip_set_update_engine": (C.c_int, [vp, C.c_int32]),
        "fiesta_hip_level_trace": (C.c_int, [vp, vp, vp]),
        "fiesta_hip_level_tuning": (C.c_int, [vp, C.c_int32, C.c_int64]),
        "fiesta_hip_count_no_obstacle": (C.c_int, [vp, vp]),
        "fiesta_hip_set_occupancy_vox": (C.c_int, [vp, vp, vp, i64, vp]),
        "fiesta_hip_set_occupancy_pos": (C.c_int, [vp, vp, vp, i64, vp]),
        "fiesta_hip_set_occupancy_vox_dev": (C.c_int, [vp, vp, vp, i64]),
        "fiesta_hip_set_occupancy_box": (C.c_int, [vp, vp, vp, i32]),
        "fiesta_hip_raycast_frame": (C.c_int, [vp, vp, i64, vp, vp, vp]),
        "fiesta_hip_raycast_frame_dev": (C.c_int, [vp, vp, i64, vp, vp, vp]),
        "fiesta_hip_raycast_depth": (C.c_int, [vp, vp, i32, i32, dbl, dbl, dbl, dbl, vp, vp, vp]),
        "fiesta_hip_raycast_depth_filtered": (C.c_int, [vp, vp, i32, i32, dbl, dbl, dbl, dbl, vp, vp, vp, vp]),
        "fiesta_hip_depth_conversion": (C.c_int, [vp, vp, i32, i32, dbl, dbl, dbl, dbl, vp, vp, vp]),
        "fiesta_hip_raycast_single": (C.c_int, [vp, vp, vp, vp, vp, i32, vp, i32]),
        "fiesta_hip_check_update": (C.c_int, [vp, vp]),
        "fiesta_hip_update_occupancy": (C.c_int, [vp, i32, vp, vp, vp]),
        "fiesta_hip_update_esdf": (C.c_int, [vp, vp]),
        "fiesta_hip_get_distance_vox": (C.c_int, [vp, vp, i64, vp]),
        "fiesta_hip_get_distance_pos": (C.c_int, [vp, vp, i64, vp]),
        "fiesta_hip_get_dist_grad": (C.c_int, [vp, vp, i64, vp, vp]),
        "fiesta_hip_get_dist_grad_dev": (C.c_int, [vp, vp, i64, vp, vp]),
        "fiesta_hip_host_cache_fetches": (C.c_int, [vp, vp]),
        "fiesta_hip_path_clearance": (C.c_int, [vp, vp, i64, vp, i64, dbl, dbl, vp]),
        "fiesta_hip_path_clearance_dev": (C.c_int, [vp, vp, i64, vp, i64, dbl, dbl, vp]),
        "fiesta_hip_path_cost": (C.c_int, [vp, vp, i64, vp, i64, dbl, dbl, vp]),
        "fiesta_hip_path_cost_dev": (C.c_int, [vp, vp, i64, vp, i64, dbl, dbl, vp]),
        "fiesta_hip_body_query": (C.c_int, [vp, vp, i32, vp, i64, dbl, vp]),
        "fiesta_hip_body_query_dev": (C.c_int, [vp, vp, i32, vp, i64, dbl, vp]),
        "fiesta_hip_articulated_query": (C.c_int, [vp, vp, vp, i32, i32, vp, i64, dbl, vp]),
        "fiesta_hip_articulated_query_dev": (C.c_int, [vp, vp, vp, i32, i32, vp, i64, dbl, vp]),
        "fiesta_hip_body_sweep": (C.c_int, [vp, vp, i32, vp, i64, vp, i64, dbl, dbl, vp]),
        "fiesta_hip_body_sweep_dev": (C.c_int, [vp, vp, i32, vp, i64, vp, i64, dbl, dbl, vp]),
        "fiesta_hip_get_frontier_voxels": (C.c_int, [vp, vp, vp, dbl, vp, vp, i64, vp]),
        "fiesta_hip_get_frontier_voxels_dev": (C.c_int, [vp, vp, vp, dbl, vp, vp, i64, vp]),
        "fiesta_hip_get_skeleton_voxels": (C.c_int, [vp, vp, vp, i32, dbl, i64, vp, vp]),
        "fiesta_hip_get_skeleton_voxels_dev": (C.c_int, [vp, vp, vp, i32, dbl, i64, vp, vp]),
        "fiesta_hip_ray_query": (C.c_int, [vp, vp, vp, i64, i32, vp]),
        "fiesta_hip_ray_query_dev": (C.c_int, [vp, vp, vp, i64, i32, vp]),
        "fiesta_hip_reach_field": (C.c_int, [vp, vp, vp, vp, i64, vp, i64, dbl, i32, i32, vp, vp]),
        "fiesta_hip_reach_field_dev": (C.c_int, [vp, vp, vp, vp, i64, vp, i64, dbl, i32, i32, vp, vp]),
        "fiesta_hip_reach_matrix": (C.c_int, [vp, vp, vp, vp, i64, vp, i64, dbl, i32, i32, i32, vp, vp]),
        "fiesta_hip_reach_matrix_dev": (C.c_int, [vp, vp, vp, vp, i64, vp, i64, dbl, i32, i32, i32, vp, vp]),
        "fiesta_hip_site_tour": (C.c_int, [vp, vp, i32, i64, i32, i32, i32, C.c_uint64, i32, vp, vp]),
        "fiesta_hip_site_tour_dev": (C.c_int, [vp, vp, i32, i64, i32, i32, i32, C.c_uint64, i32, vp, vp]),
        "fiesta_hip_reach_paths": (C.c_int, [vp, vp, vp, vp, vp, i64, i32, i32, i32, i64, vp]),
        "fiesta_hip_reach_paths_dev": (C.c_int, [vp, vp, vp, vp, vp, i64, i32, i32, i32, i64, vp]),
        "fiesta_hip_leg_paths": (C.c_int, [vp, vp, vp, vp, i64, i32, i32, i64, vp, vp]),
        "fiesta_hip_leg_paths_dev": (C.c_int, [vp, vp, vp, vp, i64, i32, i32, i64, vp, vp]),
        "fiesta_hip_free_boxes": (C.c_int, [vp, vp, vp, vp, i64, dbl, i32, i32, vp]),
        "fiesta_hip_free_boxes_dev": (C.c_int, [vp, vp, vp, vp, i64, dbl, i32, i32, vp]),
        "fiesta_hip_path_corridor": (C.c_int, [vp, vp, vp, vp, i64, vp, i64, dbl, i32, i32, i64, vp]),
        "fiesta_hip_path_corridor_dev": (C.c_int, [vp, vp, vp, vp, i64, vp, i64, dbl, i32, i32, i64, vp]),
        "fiesta_hip_path_refine": (C.c_int, [vp, vp, i64, vp, i64, vp, vp, vp]),
        "fiesta_hip_path_refine_dev": (C.c_int, [vp, vp, i64, vp, i64, vp, vp, vp]),
        "fiesta_hip_path_timing": (C.c_int, [vp, vp, i64, vp, i64, vp, vp]),
        "fiesta_hip_path_timing_dev": (C.c_int, [vp, vp, i64, vp, i64, vp, vp]),
        "fiesta_hip_corridor_bounds": (C.c_int, [vp, vp, i64, vp, i64, vp, vp, vp, vp, vp, i64, dbl, i32, vp]),
        "fiesta_hip_corridor_bounds_dev": (C.c_int, [vp, vp, i64, vp, i64, vp, vp, vp, vp, vp, i64, dbl, i32, vp]),
        "fiesta_hip_cluster_voxels": (C.c_int, [vp, vp, vp, vp, i64, i32, i32, i64, i64, vp, vp]),
        "fiesta_hip_cluster_voxels_dev": (C.c_int, [vp, vp, vp, vp, i64, vp, i32, i32, i64, i64, vp, vp]),
        "fiesta_hip_split_clusters": (C.c_int, [vp, vp, vp, vp, i64, vp, vp, i64, i64, i32, i32, i32, i64, vp, vp]),
        "fiesta_hip_split_clusters_dev": (C.c_int, [vp, vp, vp, vp, i64, vp, vp, i64, vp, i64, i32, i32, i32, i64, vp, vp]),
        "fiesta_hip_view_coverage": (C.c_int, [vp, vp, i64, vp, vp, i64, i64, vp, vp, vp, vp]),
        "fiesta_hip_view_coverage_dev": (C.c_int, [vp, vp, i64, vp, vp, i64, vp, i64, vp, vp, vp, vp]),
        "fiesta_hip_get_occupancy_vox": (C.c_int, [vp, vp, i64, vp]),
        "fiesta_hip_get_occupancy_pos": (C.c_int, [vp, vp, i64, vp]),
        "fiesta_hip_download_field": (C.c_int, [vp, vp, vp, vp, vp]),
        "fiesta_hip_download_counts": (C.c_int, [vp, vp, vp]),
        "fiesta_hip_get_occupied_voxels": (C.c_int, [vp, vp, i64, vp]),
        "fiesta_hip_get_slice": (C.c_int, [vp, i32, vp]),
        "fiesta_hip_download_hash": (C.c_int, [vp, vp, vp, vp, vp, vp]),
        "fiesta_hip_snapshot_save": (C.c_int, [vp, i32]),
        "fiesta_hip_snapshot_restore": (C.c_int, [vp, i32]),
        "fiesta_hip_snapshot_count_updated": (C.c_int, [vp, i32, vp]),
        "fiesta_hip_shard_info_get": (C.c_int, [vp, vp]),
        "fiesta_hip_halo_pack_dev": (C.c_int, [vp, vp, vp, vp]),
        "fiesta_hip_halo_apply_dev": (C.c_int, [vp, vp, vp, vp, vp]),
        "fiesta_hip_export_transitions_dev": (C.c_int, [vp, vp, i64, vp]),
        "fiesta_hip_apply_transitions_dev": (C.c_int, [vp, vp, i64]),
        "fiesta_hip_halo_pack": (C.c_int, [vp, vp, vp, vp]),
        "fiesta_hip_halo_apply": (C.c_int, [vp, vp, vp, vp, vp]),
        "fiesta_hip_export_transitions": (C.c_int, [vp, vp, i64, vp]),
        "fiesta_hip_apply_transitions": (C.c_int, [vp, vp, i64]),
        "fiesta_hip_esdf_seed": (C.c_int, [vp, vp]),
        "fiesta_hip_relax_pending": (C.c_int, [vp, vp, vp]),
        "fiesta_hip_synchronize": (C.c_int, [vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    lib._fiesta_signatures = sig
    _lib = lib
    return lib


def last_error() -> str:
    return load().fiesta_hip_last_error().decode(errors="replace")


def check(status: int):
    if status != 0:
        raise FiestaHipError(status, load().fiesta_hip_last_error().decode(errors="replace"))


def device_count() -> int:
    return int(load().fiesta_hip_device_count())
