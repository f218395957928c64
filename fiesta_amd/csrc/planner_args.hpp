// fiesta_amd/csrc/planner_args.hpp -- the planner calls' argument aggregates: one per host / _dev pair of the C ABI.
// c_api.hip builds each from the ABI's arguments and checks it; the call's kernel header takes the same object.  Plain data over the
// types of include/fiesta_hip.h: no kernel, no scratch.
#pragma once
#include <stdint.h>

#include "../../include/fiesta_hip.h"

namespace fiesta {
// the arguments as fiesta_hip_path_clearance[_dev] and fiesta_hip_path_cost[_dev] take them (R: the call's result struct),
// already checked
template <typename R>
struct PathArgs {
  const double *w;
  int64_t n_wp;
  const int64_t *off;
  int64_t n_paths;
  double step, margin;
  const R *res;
  bool dev;
};
using PathClearanceArgs = PathArgs<fiesta_hip_path_result>;
using PathCostArgs = PathArgs<fiesta_hip_path_cost_result>;

struct BodyArgs {  // the call's arguments as fiesta_hip_body_query[_dev] takes them, already checked
  const double *spheres;  // a host pointer in both variants: cx, cy, cz, r per sphere
  int32_t n_spheres;
  const double *poses;
  int64_t n_poses;
  double margin;
  const fiesta_hip_body_result *res;
  bool dev;
};

struct ArticulatedArgs {  // the call's arguments as fiesta_hip_articulated_query[_dev] takes them, already checked
  const double *spheres;        // host pointers in both variants: cx, cy, cz, r per sphere (in its frame) and the sphere's frame,
  const int32_t *sphere_frame;  // non-decreasing, 0 .. n_frames - 1
  int32_t n_spheres, n_frames;
  const double *frame_poses;  // n_configs x n_frames x 7
  int64_t n_configs;
  double margin;
  const fiesta_hip_articulated_result *res;
  bool dev;
};

struct SweepArgs {  // the call's arguments as fiesta_hip_body_sweep[_dev] takes them, already checked
  const double *spheres;  // a host pointer in both variants: cx, cy, cz, r per sphere
  int32_t n_spheres;
  const double *poses;  // the waypoint poses, n_poses x 7
  int64_t n_poses;
  const int64_t *off;
  int64_t n_paths;
  double step, margin;
  const fiesta_hip_sweep_result *res;
  bool dev;
};

struct FrontierArgs {  // the call's arguments as fiesta_hip_get_frontier_voxels[_dev] takes them, already checked
  const int32_t *lo, *hi;  // both null: the whole map
  double min_clearance;
  int32_t *vox;
  uint8_t *mask;
  int64_t capacity;
  unsigned long long *n_out_dev;  // the device variant's total
  bool dev;
};

struct SkeletonArgs {  // the call's arguments as fiesta_hip_get_skeleton_voxels[_dev] takes them, already checked
  const int32_t *lo, *hi;  // both null: the whole map
  int32_t min_sep2;
  double min_clearance;
  int64_t capacity;
  const fiesta_hip_skeleton_result *res;
  unsigned long long *n_out_dev;  // the device variant's total
  bool dev;
};

struct RayArgs {  // the call's arguments as fiesta_hip_ray_query[_dev] takes them, already checked
  const double *start, *end;
  int64_t n;
  int stop_mask;
  const fiesta_hip_ray_result *res;
  bool dev;
};

struct ReachArgs {  // the call's arguments as fiesta_hip_reach_field[_dev] takes them, already checked
  const int32_t *lo, *hi;  // the caller's box (both null: the whole array)
  const int32_t *seeds;
  int64_t n_seeds;
  const int32_t *targets;
  int64_t n_targets;
  double min_clearance;
  int connectivity, flags;
  const fiesta_hip_reach_result *res;
  fiesta_hip_reach_info *info;
  bool dev;
};

struct ReachMatrixArgs {  // the call's arguments as fiesta_hip_reach_matrix[_dev] takes them, already checked
  const int32_t *lo, *hi;  // the caller's box (both null: the whole array)
  const int32_t *sources;
  int64_t n_sources;
  const int32_t *targets;  // null with n_targets = 0: the columns are the sources
  int64_t n_targets;
  double min_clearance;
  int connectivity, flags, max_fields;
  const fiesta_hip_reach_matrix_result *res;
  fiesta_hip_reach_matrix_info *info;
  bool dev;
};

struct ReachPathArgs {  // the call's arguments as fiesta_hip_reach_paths[_dev] takes them, already checked
  const int32_t *cost;  // null: the retained field
  const int32_t *box_lo, *box_hi;
  const int32_t *targets;
  int64_t n_targets;
  int connectivity, flags, max_span;
  int64_t capacity;
  const fiesta_hip_reach_paths_result *res;
  bool dev;
};

struct LegPathArgs {  // the call's arguments as fiesta_hip_leg_paths[_dev] takes them, already checked
  const int32_t *from, *to, *to_vox;  // exactly one of to / to_vox unless n_legs = 0
  int64_t n_legs;
  int flags, max_span;
  int64_t capacity;
  const fiesta_hip_leg_paths_result *res;
  fiesta_hip_leg_paths_info *info;
  bool dev;
};

struct CorridorArgs {  // the arguments of both call pairs as the ABI takes them, already checked
  bool paths;          // fiesta_hip_path_corridor (else fiesta_hip_free_boxes)
  const int32_t *lo, *hi;  // the window (host pointers; both null: none given)
  const int32_t *vox;      // the seeds, or the waypoints
  int64_t n_vox;
  const int64_t *offsets;  // paths: CSR over the waypoints, n_paths + 1
  int64_t n_paths;
  double min_clearance;
  int max_grow, flags;
  int64_t capacity;
  const fiesta_hip_free_boxes_result *boxes;   // free boxes
  const fiesta_hip_corridor_result *corridor;  // paths
  bool dev;
};

// the arguments as fiesta_hip_path_refine[_dev] take them, already checked
struct PathRefineArgs {
  const double *w;
  int64_t n_wp;
  const int64_t *off;
  int64_t n_paths;
  const double *bounds;  // nullable
  const fiesta_hip_refine_params *par;
  const fiesta_hip_refine_result *res;
  bool dev;
};

// the arguments as fiesta_hip_path_timing[_dev] take them, already checked
struct PathTimingArgs {
  const double *w;
  int64_t n_wp;
  const int64_t *off;
  int64_t n_paths;
  const fiesta_hip_timing_params *par;
  const fiesta_hip_path_timing_result *res;
  bool dev;
};

// the arguments as fiesta_hip_corridor_bounds[_dev] take them, already checked
struct CorridorBoundsArgs {
  const int32_t *w;
  int64_t n_wp;
  const int64_t *off;
  int64_t n_paths;
  const int64_t *box_off;
  const int32_t *boxes;
  const double *boxes_pos;
  const int32_t *entry;
  const int32_t *status;
  int64_t n_boxes;
  double inset;
  int32_t flags;
  const fiesta_hip_bounds_result *res;
  bool dev;
};

struct TourArgs {  // the call's arguments as fiesta_hip_site_tour[_dev] takes them, already checked
  const int32_t *cost;
  int32_t n;
  int64_t ld;
  int32_t start, flags, restarts;
  uint64_t seed;
  int32_t max_moves;
  const fiesta_hip_tour_result *res;  // nullable
  fiesta_hip_tour_info *info;
  bool dev;
};

struct ClusterArgs {  // the call's arguments as fiesta_hip_cluster_voxels[_dev] takes them, already checked
  const int32_t *vox;
  const uint8_t *mask;
  const int32_t *key;
  int64_t n;
  const unsigned long long *n_dev;
  int connectivity, min_size;
  int64_t cluster_capacity, member_capacity;
  const fiesta_hip_cluster_result *res;
  fiesta_hip_cluster_info *info;
  bool dev;
};

struct SplitArgs {  // the call's arguments as fiesta_hip_split_clusters[_dev] takes them, already checked
  const int32_t *vox;
  const uint8_t *mask;
  const int32_t *key;
  int64_t n;
  const int64_t *offsets, *members;
  int64_t n_clusters;
  const int64_t *n_clusters_dev;
  int64_t n_members;
  int max_size, max_extent, max_depth;
  int64_t part_capacity;
  const fiesta_hip_split_result *res;
  fiesta_hip_split_info *info;
  bool dev;
};

struct ViewArgs {  // the call's arguments as fiesta_hip_view_coverage[_dev] takes them, already checked
  const int32_t *vox;
  int64_t n;
  const int64_t *offsets, *members;
  int64_t n_groups;
  const int64_t *n_groups_dev;
  int64_t n_members;
  const fiesta_hip_view_set *views;
  const fiesta_hip_view_sensor *sensor;
  const fiesta_hip_view_result *res;
  fiesta_hip_view_info *info;
  bool dev;
};

}  // namespace fiesta
