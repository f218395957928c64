"""fiesta_amd -- MI355X-native incremental ESDF engine behind FIESTA's ``ESDFMap`` operator API.

The product is ``libfiesta_hip.so`` (hand-written HIP for gfx950 behind the C ABI of
include/fiesta_hip.h); this package is the thin host-side mirror of the reference interface.
"""
from ._lib import FiestaHipError, LIB_PATH, device_count, load  # noqa: F401
from .esdf_map import (D2_INF, INFINITY, UNDEFINED, ESDFMap, frontier_model, path_cost_model, path_samples, ray_query_model,  # noqa: F401
                       ray_walk, ray_walks, signed_distance)
from .body_model import BODY_MAX_SPHERES, body_query_model, body_rotation  # noqa: F401
from .articulated_model import BODY_MAX_FRAMES, articulated_query_model, group_spheres_by_frame  # noqa: F401
from .sweep_model import body_reach, body_sweep_model, sweep_poses  # noqa: F401
from .cluster_model import cluster_model, cluster_stencil  # noqa: F401
from .skeleton_model import skeleton_model  # noqa: F401
from .split_model import SPLIT_INVALID, SPLIT_MAX_DEPTH, SPLIT_OK, split_model  # noqa: F401
from .view_model import VIEW_OMNI, view_coverage_model, view_ring  # noqa: F401
from .reach_model import (LEG_BAD_INDEX, LEG_NO_SOURCE, REACH_PATHS_SHORTCUT, REACH_THROUGH_UNKNOWN, leg_paths_model,  # noqa: F401
                          reach_matrix_model, reach_model, reach_moves, reach_paths_model, reach_visible, reach_walk)
from .corridor_model import (CORRIDOR_BLOCKED, CORRIDOR_INVALID, CORRIDOR_MAX_GROW, CORRIDOR_OK, CORRIDOR_STOP_BLOCKED,  # noqa: F401
                             CORRIDOR_STOP_EDGE, CORRIDOR_STOP_LIMIT, CORRIDOR_THROUGH_UNKNOWN, FREE_BOX_BLOCKED, FREE_BOX_OK,
                             FREE_BOX_OUTSIDE, corridor_chain, corridor_model, free_box_model)
from .refine_model import (BOUNDS_VOID_BROKEN, REFINE_INVALID, REFINE_MAX_ITERATIONS, REFINE_MAX_WAYPOINTS, REFINE_OK,  # noqa: F401
                           corridor_bounds, corridor_bounds_model, path_refine_gradient, path_refine_model)
from .tour_model import TOUR_CLOSED, best_move, tour_model  # noqa: F401
from .timing_model import (TIMING_INVALID, TIMING_MAX_SAMPLES, TIMING_MAX_WAYPOINTS, TIMING_OK, TIMING_TOO_LONG,  # noqa: F401
                           path_timing_model)

__all__ = ["body_reach", "sweep_poses", "body_sweep_model", "articulated_query_model", "group_spheres_by_frame", "BODY_MAX_FRAMES", "body_query_model","body_rotation", "BODY_MAX_SPHERES", "path_timing_model", "TIMING_OK", "TIMING_INVALID", "TIMING_TOO_LONG", "TIMING_MAX_WAYPOINTS", "TIMING_MAX_SAMPLES", "path_refine_model", "path_refine_gradient", "corridor_bounds", "corridor_bounds_model", "BOUNDS_VOID_BROKEN","REFINE_OK", "REFINE_INVALID", "REFINE_MAX_WAYPOINTS",
           "REFINE_MAX_ITERATIONS", "free_box_model", "corridor_chain", "corridor_model", "CORRIDOR_THROUGH_UNKNOWN", "CORRIDOR_MAX_GROW", "CORRIDOR_STOP_BLOCKED",
           "CORRIDOR_STOP_EDGE", "CORRIDOR_STOP_LIMIT", "FREE_BOX_OK", "FREE_BOX_OUTSIDE", "FREE_BOX_BLOCKED", "CORRIDOR_OK", "CORRIDOR_INVALID",
           "CORRIDOR_BLOCKED", "tour_model", "best_move", "TOUR_CLOSED", "ESDFMap", "signed_distance", "path_samples", "path_cost_model", "frontier_model", "ray_walk", "ray_walks", "ray_query_model", "reach_model", "reach_matrix_model", "REACH_THROUGH_UNKNOWN", "reach_moves", "reach_paths_model", "leg_paths_model", "LEG_NO_SOURCE", "LEG_BAD_INDEX", "reach_visible", "reach_walk", "REACH_PATHS_SHORTCUT", "cluster_model", "cluster_stencil", "skeleton_model", "split_model", "SPLIT_OK", "SPLIT_INVALID", "SPLIT_MAX_DEPTH", "view_coverage_model", "view_ring", "VIEW_OMNI", "FiestaHipError", "device_count", "load", "LIB_PATH", "UNDEFINED", "INFINITY",
           "D2_INF"]
