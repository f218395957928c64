// fiesta_amd/csrc/c_api.hip -- the extern "C" boundary declared in include/fiesta_hip.h.
// Every entry point converts C++ exceptions into a status code + thread-local message; nothing throws
// across the ABI and no HIP / C++ type appears in a signature.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "../../include/fiesta_hip.h"
#include "dense_map.hpp"
#include "dense_read.hpp"
#include "hash_map.hpp"
#include "hash_read.hpp"
#include "planner.hpp"
#include "planner_args.hpp"
#include "shard_group.hpp"

using fiesta::DenseMap;
using fiesta::Error;
using fiesta::HashMap;

struct fiesta_hip_shard_group {
  fiesta::ShardGroup *g = nullptr;
};

struct fiesta_hip_map {
  int mode = 0;
  DenseMap *dense = nullptr;
  HashMap *hash = nullptr;
};

namespace {
thread_local std::string g_last_error;

template <typename F>
int guarded(F &&f) {
  try {
    f();
    return FIESTA_HIP_OK;
  } catch (const Error &e) {
    g_last_error = e.what();
    return e.code;
  } catch (const std::exception &e) {
    g_last_error = e.what();
    return FIESTA_HIP_ERR_DEVICE;
  } catch (...) {
    g_last_error = "unknown error";
    return FIESTA_HIP_ERR_DEVICE;
  }
}
void need(bool ok, const char *msg) {
  if (!ok) throw Error(FIESTA_HIP_ERR_INVALID, msg);
}
// f on the map's store: f(DenseMap &) or f(HashMap &), whichever the handle holds
template <typename F>
auto on_store(fiesta_hip_map *m, F &&f) {
  return m->dense ? f(*m->dense) : f(*m->hash);
}
DenseMap &dense(fiesta_hip_map *m, const char *what) {
  need(m != nullptr, "null map handle");
  if (!m->dense) throw Error(FIESTA_HIP_ERR_INVALID, std::string(what) + ": only available on array-mode maps");
  return *m->dense;
}
// The planner calls: one body per host / _dev pair.  Each checks the whole-call errors of include/fiesta_hip.h on the arguments as
// the ABI took them (the call's aggregate of planner_args.hpp), then hands the same object on to the call's function of planner.hpp,
// with the store's planner_ctx() and -- the fourteen calls that read voxels -- its planner_view(does the call read the bitmaps?).

// shared by path_clearance and path_cost (R: the call's result struct); a host batch: the CSR rules as well
template <typename R>
void path_checks(fiesta_hip_map *m, const fiesta::PathArgs<R> &a) {
  need(m && a.w && a.off && a.res, "null argument");
  need(a.n_wp >= 0 && a.n_paths >= 0, "negative count");
  need(std::isfinite(a.step) && a.step > 0, "path query: step must be finite and > 0");
  need(!std::isnan(a.margin), "path query: margin is NaN");
  if (a.dev) return;
  need(a.off[0] == 0 && a.off[a.n_paths] == a.n_wp, "path query: offsets[0] must be 0 and offsets[n_paths] = n_waypoints");
  for (int64_t p = 0; p < a.n_paths; ++p) need(a.off[p] <= a.off[p + 1], "path query: offsets must be non-decreasing");
}
void path_clearance(fiesta_hip_map *m, const fiesta::PathClearanceArgs &a) {
  path_checks(m, a);
  on_store(m, [&](auto &s) { fiesta::path_clearance(s.planner_ctx(), s.planner_view(false), s.host_path_eval(), a); });
}
void path_cost(fiesta_hip_map *m, const fiesta::PathCostArgs &a) {
  path_checks(m, a);
  need(std::isfinite(a.margin), "path_cost: margin must be finite");
  on_store(m, [&](auto &s) { fiesta::path_cost(s.planner_ctx(), s.planner_view(false), s.host_path_eval(), a); });
}
// fiesta_hip_body_query: none of these errors needs a device; the sphere table is a host pointer in both variants and is checked here
void body_query(fiesta_hip_map *m, const fiesta::BodyArgs &a) {
  need(m != nullptr, "null map handle");
  need(a.n_spheres >= 1 && a.n_spheres <= FIESTA_HIP_BODY_MAX_SPHERES, "body_query: n_spheres must be 1 .. 1024");
  need(a.n_poses >= 0, "body_query: negative count");
  need(a.spheres != nullptr, "body_query: spheres is null");
  need(a.poses != nullptr || a.n_poses == 0, "body_query: poses is null");
  need(a.res != nullptr, "body_query: result is null");
  for (int64_t i = 0; i < 4 * (int64_t)a.n_spheres; ++i) need(std::isfinite(a.spheres[i]), "body_query: a sphere's centre or radius is not finite");
  for (int32_t i = 0; i < a.n_spheres; ++i) need(a.spheres[4 * i + 3] >= 0, "body_query: a sphere's radius is negative");
  need(std::isfinite(a.margin), "body_query: margin must be finite");
  on_store(m, [&](auto &s) { fiesta::body_query(s.planner_ctx(), s.planner_view(false), a); });
}
// fiesta_hip_articulated_query: as body_query; the sphere table and its frame indices are host pointers in both variants
void articulated_query(fiesta_hip_map *m, const fiesta::ArticulatedArgs &a) {
  need(m != nullptr, "null map handle");
  need(a.n_spheres >= 1 && a.n_spheres <= FIESTA_HIP_BODY_MAX_SPHERES, "articulated_query: n_spheres must be 1 .. 1024");
  need(a.n_frames >= 1 && a.n_frames <= FIESTA_HIP_BODY_MAX_FRAMES, "articulated_query: n_frames must be 1 .. 64");
  need(a.n_configs >= 0, "articulated_query: negative count");
  need(a.spheres != nullptr, "articulated_query: spheres is null");
  need(a.sphere_frame != nullptr, "articulated_query: sphere_frame is null");
  need(a.frame_poses != nullptr || a.n_configs == 0, "articulated_query: frame_poses is null");
  need(a.res != nullptr, "articulated_query: result is null");
  for (int64_t i = 0; i < 4 * (int64_t)a.n_spheres; ++i)
    need(std::isfinite(a.spheres[i]), "articulated_query: a sphere's centre or radius is not finite");
  for (int32_t i = 0; i < a.n_spheres; ++i) need(a.spheres[4 * i + 3] >= 0, "articulated_query: a sphere's radius is negative");
  for (int32_t i = 0; i < a.n_spheres; ++i)
    need(a.sphere_frame[i] >= 0 && a.sphere_frame[i] < a.n_frames, "articulated_query: a frame index is outside 0 .. n_frames - 1");
  for (int32_t i = 1; i < a.n_spheres; ++i)
    need(a.sphere_frame[i] >= a.sphere_frame[i - 1], "articulated_query: the spheres are not grouped by frame (sphere_frame decreases)");
  need(std::isfinite(a.margin), "articulated_query: margin must be finite");
  on_store(m, [&](auto &s) { fiesta::articulated_query(s.planner_ctx(), s.planner_view(false), a); });
}
// fiesta_hip_body_sweep: the body query's errors on the table and the margin, path clearance's on step, offsets and null pointers
void body_sweep(fiesta_hip_map *m, const fiesta::SweepArgs &a) {
  need(m && a.spheres && a.poses && a.off && a.res, "null argument");
  need(a.n_spheres >= 1 && a.n_spheres <= FIESTA_HIP_BODY_MAX_SPHERES, "body_sweep: n_spheres must be 1 .. 1024");
  need(a.n_poses >= 0 && a.n_paths >= 0, "negative count");
  for (int64_t i = 0; i < 4 * (int64_t)a.n_spheres; ++i) need(std::isfinite(a.spheres[i]), "body_sweep: a sphere's centre or radius is not finite");
  for (int32_t i = 0; i < a.n_spheres; ++i) need(a.spheres[4 * i + 3] >= 0, "body_sweep: a sphere's radius is negative");
  need(std::isfinite(a.step) && a.step > 0, "body_sweep: step must be finite and > 0");
  need(std::isfinite(a.margin), "body_sweep: margin must be finite");
  if (!a.dev) {
    need(a.off[0] == 0 && a.off[a.n_paths] == a.n_poses, "body_sweep: offsets[0] must be 0 and offsets[n_paths] = n_poses");
    for (int64_t p = 0; p < a.n_paths; ++p) need(a.off[p] <= a.off[p + 1], "body_sweep: offsets must be non-decreasing");
  }
  on_store(m, [&](auto &s) { fiesta::body_sweep(s.planner_ctx(), s.planner_view(false), a); });
}
// n_out: the variant's total (host or device pointer); returns the host variant's total
int64_t frontier_voxels(fiesta_hip_map *m, const fiesta::FrontierArgs &a, const void *n_out) {
  need(m != nullptr, "null map handle");
  need(n_out != nullptr, "get_frontier_voxels: n_out is null");
  need(!std::isnan(a.min_clearance), "get_frontier_voxels: min_clearance is NaN");
  need((a.lo == nullptr) == (a.hi == nullptr), "get_frontier_voxels: lo and hi must both be given or both be null");
  need(a.capacity >= 0, "get_frontier_voxels: negative capacity");
  return on_store(m, [&](auto &s) { return fiesta::frontier_voxels(s.planner_ctx(), s.planner_view(true), a); });
}
// as frontier_voxels; none of these errors needs a device
int64_t skeleton_voxels(fiesta_hip_map *m, const fiesta::SkeletonArgs &a, const void *n_out) {
  need(a.res != nullptr, "get_skeleton_voxels: result is null");
  need(n_out != nullptr, "get_skeleton_voxels: n_out is null");
  need(a.min_sep2 >= 1, "get_skeleton_voxels: min_sep2 must be at least 1");
  need(!std::isnan(a.min_clearance), "get_skeleton_voxels: min_clearance is NaN");
  need((a.lo == nullptr) == (a.hi == nullptr), "get_skeleton_voxels: lo and hi must both be given or both be null");
  need(a.capacity >= 0, "get_skeleton_voxels: negative capacity");
  need(m != nullptr, "null map handle");
  return on_store(m, [&](auto &s) { return fiesta::skeleton_voxels(s.planner_ctx(), s.planner_view(true), a); });
}
void ray_query(fiesta_hip_map *m, const fiesta::RayArgs &a) {
  need(m != nullptr, "null map handle");
  need(a.start && a.end && a.res, "ray_query: start, end or result is null");
  need(a.n >= 0, "ray_query: negative count");
  need(a.stop_mask >= 0 && a.stop_mask <= 7, "ray_query: stop_mask must be a subset of OCCUPIED | UNKNOWN | OUTSIDE (0..7)");
  on_store(m, [&](auto &s) { fiesta::ray_query(s.planner_ctx(), s.planner_view(true), a); });
}
// none of these errors needs a device: they are checked before the handle is touched; the clipped box's volume is checked by the
// map, before anything is launched
void reach_field(fiesta_hip_map *m, const fiesta::ReachArgs &a) {
  need(a.res != nullptr, "reach_field: result is null");
  need(!std::isnan(a.min_clearance), "reach_field: min_clearance is NaN");
  need((a.lo == nullptr) == (a.hi == nullptr), "reach_field: lo and hi must both be given or both be null");
  need(a.connectivity == 6 || a.connectivity == 26, "reach_field: connectivity must be 6 or 26");
  need((a.flags & ~FIESTA_HIP_REACH_THROUGH_UNKNOWN) == 0, "reach_field: unknown flag bits");
  need(a.n_seeds >= 0 && a.n_targets >= 0, "reach_field: negative count");
  need(a.seeds != nullptr || a.n_seeds == 0, "reach_field: seeds is null");
  need(a.targets != nullptr || a.n_targets == 0, "reach_field: targets is null");
  need(a.targets != nullptr || a.res->target_cost == nullptr, "reach_field: target_cost given without targets");
  need(m != nullptr, "null map handle");
  need(m->dense != nullptr || a.lo != nullptr, "reach_field: a hash-block map has no outside, the box is mandatory");
  on_store(m, [&](auto &s) { fiesta::reach_field(s.planner_ctx(), s.planner_view(true), a); });
}
// reach_field's list and the matrix's own; none needs a device
void reach_matrix(fiesta_hip_map *m, const fiesta::ReachMatrixArgs &a) {
  need(a.res != nullptr, "reach_matrix: result is null");
  need(!std::isnan(a.min_clearance), "reach_matrix: min_clearance is NaN");
  need((a.lo == nullptr) == (a.hi == nullptr), "reach_matrix: lo and hi must both be given or both be null");
  need(a.connectivity == 6 || a.connectivity == 26, "reach_matrix: connectivity must be 6 or 26");
  need((a.flags & ~FIESTA_HIP_REACH_THROUGH_UNKNOWN) == 0, "reach_matrix: unknown flag bits");
  need(a.max_fields >= 0, "reach_matrix: max_fields is negative");
  need(a.n_sources >= 0 && a.n_targets >= 0, "reach_matrix: negative count");
  need(a.sources != nullptr || a.n_sources == 0, "reach_matrix: sources is null");
  need(a.targets != nullptr || a.n_targets == 0, "reach_matrix: targets is null");
  constexpr int64_t cap = 1ll << 28;  // (each factor is tested first: the product of two such factors cannot overflow)
  const int64_t n_cols = a.targets ? a.n_targets : a.n_sources;
  need(a.n_sources <= cap && n_cols <= cap && a.n_sources * n_cols <= cap, "reach_matrix: the matrix holds more than 2^28 entries");
  need(m != nullptr, "null map handle");
  need(m->dense != nullptr || a.lo != nullptr, "reach_matrix: a hash-block map has no outside, the box is mandatory");
  on_store(m, [&](auto &s) { fiesta::reach_matrix(s.planner_ctx(), s.planner_view(true), a); });
}
// none of these errors needs a device; what the matrix itself must satisfy is checked on the device, before any search
void site_tour(fiesta_hip_map *m, const fiesta::TourArgs &a) {
  need(a.cost != nullptr, "site_tour: cost is null");
  need(a.n >= 1 && a.n <= FIESTA_HIP_TOUR_MAX_SITES, "site_tour: n must be 1 .. 512");
  need(a.start >= 0 && a.start < a.n, "site_tour: start is no site");
  need(a.ld >= a.n, "site_tour: ld is below n");
  need(a.restarts >= 1 && a.restarts <= FIESTA_HIP_TOUR_MAX_RESTARTS, "site_tour: restarts must be 1 .. 4096");
  need((a.flags & ~FIESTA_HIP_TOUR_CLOSED) == 0, "site_tour: unknown flag bits");
  need(a.max_moves >= 0, "site_tour: max_moves is negative");
  need(m != nullptr, "null map handle");
  fiesta::site_tour(on_store(m, [](auto &s) { return s.planner_ctx(); }), a);
}
// none of these errors needs a device, and all but the last are checked before the handle is touched
void reach_paths(fiesta_hip_map *m, const fiesta::ReachPathArgs &a) {
  need(a.res != nullptr, "reach_paths: result is null");
  need(a.res->offsets != nullptr, "reach_paths: result->offsets is null");
  need(a.connectivity == 6 || a.connectivity == 26, "reach_paths: connectivity must be 6 or 26");
  need((a.flags & ~FIESTA_HIP_REACH_PATHS_SHORTCUT) == 0, "reach_paths: unknown flag bits");
  need(!(a.flags & FIESTA_HIP_REACH_PATHS_SHORTCUT) || a.max_span >= 1, "reach_paths: max_span must be >= 1 with SHORTCUT");
  need(a.n_targets >= 0, "reach_paths: negative count");
  need(a.capacity >= 0, "reach_paths: negative capacity");
  need(a.targets != nullptr || a.n_targets == 0, "reach_paths: targets is null");
  need((a.cost == nullptr) == (a.box_lo == nullptr) && (a.box_lo == nullptr) == (a.box_hi == nullptr),
       "reach_paths: cost, box_lo and box_hi must all be given or all be null");
  if (a.cost) {
    int64_t nvox = 1;
    for (int c = 0; c < 3; ++c) {
      need(a.box_lo[c] <= a.box_hi[c], "reach_paths: the box is empty (box_lo > box_hi)");
      nvox *= std::min<int64_t>((int64_t)a.box_hi[c] - a.box_lo[c] + 1, (1ll << 28) + 1);  // (three factors of at most 2^28 + 1 would overflow:
      need(nvox <= (1ll << 28), "reach_paths: the box holds more than 2^28 voxels");       //  checked after every factor)
    }
  }
  need(m != nullptr, "null map handle");
  fiesta::reach_paths(on_store(m, [](auto &s) { return s.planner_ctx(); }), a);
}
// none of these errors needs a device, and all are checked before the handle is touched; whether a batch is retained is the map's to say
void leg_paths(fiesta_hip_map *m, const fiesta::LegPathArgs &a) {
  need(a.res != nullptr, "leg_paths: result is null");
  need(a.res->offsets != nullptr, "leg_paths: result->offsets is null");
  need(a.n_legs >= 0, "leg_paths: negative count");
  need(a.capacity >= 0, "leg_paths: negative capacity");
  need((a.flags & ~FIESTA_HIP_REACH_PATHS_SHORTCUT) == 0, "leg_paths: unknown flag bits");
  need(!(a.flags & FIESTA_HIP_REACH_PATHS_SHORTCUT) || a.max_span >= 1, "leg_paths: max_span must be >= 1 with SHORTCUT");
  need(a.from != nullptr || a.n_legs == 0, "leg_paths: from is null");
  need((a.to != nullptr) != (a.to_vox != nullptr) || a.n_legs == 0, "leg_paths: exactly one of to and to_vox must be given");
  need(m != nullptr, "null map handle");
  fiesta::leg_paths(on_store(m, [](auto &s) { return s.planner_ctx(); }), a);
}
// fiesta_hip_free_boxes and fiesta_hip_path_corridor: none of these errors needs a device, and all are checked before the handle
// is touched (a host batch: the CSR rules as well)
constexpr const char *kFreeBoxNames[] = {"free_boxes: result is null", "free_boxes: min_clearance is NaN",
                                         "free_boxes: lo and hi must both be given or both be null", "free_boxes: max_grow must lie in 0 .. 256",
                                         "free_boxes: unknown flag bits", "free_boxes: negative count", "free_boxes: seeds is null"};
constexpr const char *kCorridorNames[] = {"path_corridor: result is null", "path_corridor: min_clearance is NaN",
                                          "path_corridor: lo and hi must both be given or both be null", "path_corridor: max_grow must lie in 0 .. 256",
                                          "path_corridor: unknown flag bits", "path_corridor: negative count", "path_corridor: waypoints_vox is null"};
void corridor(fiesta_hip_map *m, const fiesta::CorridorArgs &a) {
  const char *const *s = a.paths ? kCorridorNames : kFreeBoxNames;
  need(a.paths ? a.corridor != nullptr : a.boxes != nullptr, s[0]);
  if (a.paths) need(a.corridor->offsets != nullptr, "path_corridor: result->offsets is null");
  need(!std::isnan(a.min_clearance), s[1]);
  need((a.lo == nullptr) == (a.hi == nullptr), s[2]);
  need(a.max_grow >= 0 && a.max_grow <= FIESTA_HIP_CORRIDOR_MAX_GROW, s[3]);
  need((a.flags & ~FIESTA_HIP_CORRIDOR_THROUGH_UNKNOWN) == 0, s[4]);
  need(a.n_vox >= 0 && a.n_paths >= 0, s[5]);
  need(a.vox != nullptr || a.n_vox == 0, s[6]);
  if (a.paths) {
    need(a.capacity >= 0, "path_corridor: negative capacity");
    need(a.offsets != nullptr, "path_corridor: offsets is null");
    if (!a.dev) {
      need(a.offsets[0] >= 0 && a.offsets[a.n_paths] <= a.n_vox, "path_corridor: offsets must lie in 0 .. n_waypoints");
      for (int64_t p = 0; p < a.n_paths; ++p) need(a.offsets[p] <= a.offsets[p + 1], "path_corridor: offsets must be non-decreasing");
    }
  }
  need(m != nullptr, "null map handle");
  on_store(m, [&](auto &st) { fiesta::corridor(st.planner_ctx(), st.planner_view(true), a); });
}
// fiesta_hip_path_refine: none of these errors needs a device, and all are checked before the handle is touched (a host batch: the
// CSR rules as well)
void path_refine(fiesta_hip_map *m, const fiesta::PathRefineArgs &a) {
  constexpr double lim = 1048576.0;  // 2^20
  need(a.w && a.off && a.par && a.res, "path_refine: waypoints, offsets, params or result is null");
  need(a.n_wp >= 0 && a.n_paths >= 0, "path_refine: negative count");
  need(a.n_paths <= (1ll << 30), "path_refine: more than 2^30 paths");
  const fiesta_hip_refine_params &p = *a.par;
  need(std::isfinite(p.margin) && std::fabs(p.margin) <= lim, "path_refine: margin must be finite, |margin| <= 2^20");
  need(p.w_obstacle >= 0 && p.w_obstacle <= lim, "path_refine: w_obstacle must lie in 0 .. 2^20");  // (a NaN fails every comparison)
  need(p.w_smooth >= 0 && p.w_smooth <= lim, "path_refine: w_smooth must lie in 0 .. 2^20");
  need(p.alpha > 0 && p.alpha <= lim, "path_refine: alpha must be > 0 and <= 2^20");
  need(p.max_step > 0 && p.max_step <= lim, "path_refine: max_step must be > 0 and <= 2^20");
  need(std::isfinite(p.tolerance) && p.tolerance >= 0, "path_refine: tolerance must be finite and >= 0");
  need(p.iterations >= 0 && p.iterations <= FIESTA_HIP_REFINE_MAX_ITERATIONS, "path_refine: iterations must lie in 0 .. 1024");
  need(p.flags == 0, "path_refine: flags must be 0");
  if (!a.dev) {
    need(a.off[0] == 0 && a.off[a.n_paths] == a.n_wp, "path_refine: offsets[0] must be 0 and offsets[n_paths] = n_waypoints");
    for (int64_t i = 0; i < a.n_paths; ++i) need(a.off[i] <= a.off[i + 1], "path_refine: offsets must be non-decreasing");
  }
  need(m != nullptr, "null map handle");
  on_store(m, [&](auto &s) { fiesta::path_refine(s.planner_ctx(), s.planner_view(false), a); });
}
// fiesta_hip_path_timing: none of these errors needs a device, and all are checked before the handle is touched (a host batch: the
// CSR rules as well)
void path_timing(fiesta_hip_map *m, const fiesta::PathTimingArgs &a) {
  need(a.w && a.off && a.par && a.res, "path_timing: waypoints, offsets, params or result is null");
  need(a.n_wp >= 0 && a.n_paths >= 0, "path_timing: negative count");
  need(a.n_paths <= (1ll << 30), "path_timing: more than 2^30 paths");
  const fiesta_hip_timing_params &p = *a.par;
  need(std::isfinite(p.step) && p.step > 0, "path_timing: step must be finite and > 0");
  need(std::isfinite(p.margin) && p.margin >= 0, "path_timing: margin must be finite and >= 0");
  need(std::isfinite(p.v_max) && p.v_max > 0, "path_timing: v_max must be finite and > 0");
  need(std::isfinite(p.v_min) && p.v_min > 0 && p.v_min <= p.v_max, "path_timing: v_min must be finite, 0 < v_min <= v_max");
  need(std::isfinite(p.a_max) && p.a_max > 0, "path_timing: a_max must be finite and > 0");
  need(p.corner_dev > 0, "path_timing: corner_dev must be > 0 (+inf: no corner rule)");  // (a NaN fails the comparison)
  need(std::isfinite(p.v_start) && p.v_start >= 0, "path_timing: v_start must be finite and >= 0");
  need(std::isfinite(p.v_end) && p.v_end >= 0, "path_timing: v_end must be finite and >= 0");
  if (!a.dev) {
    need(a.off[0] == 0 && a.off[a.n_paths] == a.n_wp, "path_timing: offsets[0] must be 0 and offsets[n_paths] = n_waypoints");
    for (int64_t i = 0; i < a.n_paths; ++i) need(a.off[i] <= a.off[i + 1], "path_timing: offsets must be non-decreasing");
  }
  need(m != nullptr, "null map handle");
  on_store(m, [&](auto &s) { fiesta::path_timing(s.planner_ctx(), s.planner_view(false), a); });
}
// fiesta_hip_corridor_bounds: none of these errors needs a device, and all are checked before the handle is touched (a host batch:
// the CSR rules of both offset arrays as well)
void corridor_bounds(fiesta_hip_map *m, const fiesta::CorridorBoundsArgs &a) {
  need(a.res != nullptr, "corridor_bounds: result is null");
  need(a.n_wp >= 0 && a.n_paths >= 0 && a.n_boxes >= 0, "corridor_bounds: negative count");
  need(a.n_paths <= (1ll << 30), "corridor_bounds: more than 2^30 paths");
  need(a.w != nullptr || a.n_wp == 0, "corridor_bounds: waypoints_vox is null");
  need((a.off && a.box_off && a.status) || a.n_paths == 0, "corridor_bounds: offsets, box_offsets or status is null");
  need((a.boxes && a.boxes_pos && a.entry) || a.n_boxes == 0, "corridor_bounds: boxes, boxes_pos or entry is null");
  need(std::isfinite(a.inset) && a.inset >= 0, "corridor_bounds: inset must be finite and >= 0");
  need((a.flags & ~FIESTA_HIP_BOUNDS_VOID_BROKEN) == 0, "corridor_bounds: unknown flag bits");
  if (!a.dev && a.n_paths > 0) {
    need(a.off[0] == 0 && a.off[a.n_paths] == a.n_wp, "corridor_bounds: offsets[0] must be 0 and offsets[n_paths] = n_waypoints");
    for (int64_t i = 0; i < a.n_paths; ++i) {
      need(a.off[i] <= a.off[i + 1], "corridor_bounds: offsets must be non-decreasing");
      need(a.box_off[i] >= 0 && a.box_off[i] <= a.box_off[i + 1] && a.box_off[i + 1] <= a.n_boxes,
           "corridor_bounds: a box range decreases, is negative or ends above n_boxes");
    }
  }
  need(m != nullptr, "null map handle");
  fiesta::corridor_bounds(on_store(m, [](auto &s) { return s.planner_ctx(); }), a);
}
// none of these errors needs a device
void cluster_voxels(fiesta_hip_map *m, const fiesta::ClusterArgs &a) {
  need(a.info != nullptr, "cluster_voxels: info is null");
  need(a.n >= 0 && a.n <= (1ll << 24), "cluster_voxels: the entry count must lie in 0 .. 2^24");
  need(a.connectivity == 6 || a.connectivity == 18 || a.connectivity == 26, "cluster_voxels: connectivity must be 6, 18 or 26");
  need(a.min_size >= 1, "cluster_voxels: min_size must be >= 1");
  need(a.cluster_capacity >= 0 && a.member_capacity >= 0, "cluster_voxels: negative capacity");
  need(a.vox != nullptr || a.n == 0, "cluster_voxels: vox is null");
  need(m != nullptr, "null map handle");
  fiesta::cluster_voxels(on_store(m, [](auto &s) { return s.planner_ctx(); }), a);
}
// fiesta_hip_split_clusters: none of these errors needs a device, and all are checked before the handle is touched (a host batch: the
// data errors as well -- the _dev variant finds those on the device and reports them in info.status)
void split_clusters(fiesta_hip_map *m, const fiesta::SplitArgs &a) {
  constexpr int64_t cap = 1ll << 24;
  need(a.info != nullptr, "split_clusters: info is null");
  need(a.n >= 0 && a.n <= cap, "split_clusters: the entry count must lie in 0 .. 2^24");
  need(a.n_clusters >= 0 && a.n_clusters <= cap, "split_clusters: the cluster count must lie in 0 .. 2^24");
  need(a.n_members >= 0 && a.n_members <= cap, "split_clusters: the member count must lie in 0 .. 2^24");
  need(a.max_size >= 0, "split_clusters: max_size must be >= 0");
  need(a.max_extent >= 0, "split_clusters: max_extent must be >= 0");
  need(a.max_depth >= 0 && a.max_depth <= FIESTA_HIP_SPLIT_MAX_DEPTH, "split_clusters: max_depth must lie in 0 .. 63");
  need(a.part_capacity >= 0, "split_clusters: negative capacity");
  need(a.vox != nullptr || a.n == 0, "split_clusters: vox is null");
  need(a.offsets != nullptr || a.n_clusters == 0, "split_clusters: offsets is null");
  need(a.members != nullptr || a.n_members == 0, "split_clusters: members is null");
  if (!a.dev && a.n_clusters > 0) {
    const int64_t m0 = a.offsets[0], m1 = a.offsets[a.n_clusters];
    need(m0 >= 0, "split_clusters: offsets[0] is negative");
    need(m1 <= a.n_members, "split_clusters: offsets[n_clusters] is above n_members");
    for (int64_t k = 0; k < a.n_clusters; ++k) need(a.offsets[k] <= a.offsets[k + 1], "split_clusters: offsets must be non-decreasing");
    constexpr int lim = (1 << 20) - 1;
    for (int64_t j = m0; j < m1; ++j) {
      const int64_t i = a.members[j];
      need(i >= 0 && i < a.n, "split_clusters: a member index lies outside the entry list");
      const int32_t *v = a.vox + 3 * i;
      need(v[0] > -lim && v[0] < lim && v[1] > -lim && v[1] < lim && v[2] > -lim && v[2] < lim,
           "split_clusters: a member's voxel breaks the coordinate limit (|c| < 2^20 - 1)");
    }
  }
  need(m != nullptr, "null map handle");
  fiesta::split_clusters(on_store(m, [](auto &s) { return s.planner_ctx(); }), a);
}
// none of these errors needs a device
void view_coverage(fiesta_hip_map *m, const fiesta::ViewArgs &a) {
  constexpr int64_t cap = 1ll << 24;
  const fiesta_hip_view_set *views = a.views;
  const fiesta_hip_view_sensor *s = a.sensor;
  need(views != nullptr && s != nullptr, "view_coverage: views or sensor is null");
  need(a.info != nullptr, "view_coverage: info is null");
  need(a.n >= 0 && a.n <= cap, "view_coverage: the entry count must lie in 0 .. 2^24");
  need(a.n_groups >= 0 && a.n_groups <= cap, "view_coverage: the group count must lie in 0 .. 2^24");
  need(a.members == nullptr || (a.n_members >= 0 && a.n_members <= cap), "view_coverage: the member count must lie in 0 .. 2^24");  // (ignored without members)
  need(a.vox != nullptr || a.n == 0, "view_coverage: vox is null");
  need((views->pos != nullptr) != (views->centroid != nullptr), "view_coverage: exactly one view form (pos, or centroid and ring) must be given");
  const bool omni = (s->flags & FIESTA_HIP_VIEW_OMNI) != 0;
  if (views->pos) {
    need(views->n_views >= 0 && views->n_views <= cap, "view_coverage: the view count must lie in 0 .. 2^24");
    need(views->dir != nullptr || omni, "view_coverage: dir is null without FIESTA_HIP_VIEW_OMNI");
  } else {
    need(views->ring != nullptr && views->n_ring >= 0 && views->n_ring <= cap, "view_coverage: the ring form needs ring and 0 <= n_ring <= 2^24");
    need((a.offsets ? a.n_groups : 1) * views->n_ring <= cap, "view_coverage: the view count must lie in 0 .. 2^24");
  }
  // (a NaN fails every comparison)
  need(s->min_range >= 0 && s->max_range >= 0 && s->min_range <= s->max_range, "view_coverage: the range must satisfy 0 <= min_range <= max_range");
  need(s->tan_h >= 0 && s->tan_v >= 0, "view_coverage: the tangents must be >= 0");
  need(s->min_clearance == s->min_clearance, "view_coverage: min_clearance is NaN");
  need(s->block_mask >= 0 && s->block_mask <= 7, "view_coverage: block_mask must be a subset of OCCUPIED | UNKNOWN | OUTSIDE");
  need((s->flags & ~FIESTA_HIP_VIEW_OMNI) == 0, "view_coverage: unknown flag bits");
  need(s->min_visible >= 1, "view_coverage: min_visible must be >= 1");
  need(m != nullptr, "null map handle");
  on_store(m, [&](auto &st) { fiesta::view_coverage(st.planner_ctx(), st.planner_view(true), a); });
}
}  // namespace

extern "C" {

const char *fiesta_hip_last_error(void) { return g_last_error.c_str(); }
int fiesta_hip_version(void) { return 101; }

int fiesta_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  int ok = 0;
  for (int i = 0; i < n; ++i) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, i) == hipSuccess && std::strncmp(p.gcnArchName, "gfx950", 6) == 0) ++ok;
  }
  return ok;
}

int fiesta_hip_create(const fiesta_hip_config *cfg, fiesta_hip_map **out) {
  return guarded([&] {
    need(cfg && out, "null argument");
    *out = nullptr;
    auto *m = new fiesta_hip_map;
    try {
      m->mode = cfg->mode;
      if (cfg->mode == FIESTA_HIP_MODE_ARRAY)
        m->dense = new DenseMap(*cfg);
      else if (cfg->mode == FIESTA_HIP_MODE_HASH)
        m->hash = new HashMap(*cfg);
      else
        throw Error(FIESTA_HIP_ERR_INVALID, "unknown mode");
    } catch (...) {
      delete m;
      throw;
    }
    *out = m;
  });
}

int fiesta_hip_destroy(fiesta_hip_map *m) {
  return guarded([&] {
    if (!m) return;
    delete m->dense;
    delete m->hash;
    delete m;
  });
}

int fiesta_hip_grid_size(fiesta_hip_map *m, int32_t out[3]) {
  return guarded([&] {
    need(m && out, "null argument");
    if (m->dense) {
      out[0] = m->dense->geom().nx;
      out[1] = m->dense->geom().ny;
      out[2] = m->dense->geom().nz;
    } else {
      out[0] = out[1] = out[2] = 0;
    }
  });
}
int fiesta_hip_grid_total_size(fiesta_hip_map *m, int64_t *out) {
  return guarded([&] {
    need(m && out, "null argument");
    *out = m->dense ? m->dense->total() : m->hash->allocated_voxels();  // (two different questions: nothing to share)
  });
}

int fiesta_hip_voxel_key(fiesta_hip_map *m, const int32_t *vox, int64_t n, int32_t *out) {
  return guarded([&] {
    need(m && (n == 0 || (vox && out)), "null argument");
    for (int64_t i = 0; i < n; ++i) {
      const int32_t *v = vox + 3 * i;
      if (m->dense) {
        const fiesta::Geom &g = m->dense->geom();
        out[i] = (v[0] - g.gx0) * g.ny * g.nz + (v[1] - g.gy0) * g.nz + (v[2] - g.gz0);
      } else {
        out[i] = HashMap::voxel_key(v[0], v[1], v[2]);
      }
    }
  });
}

int fiesta_hip_hash_window(fiesta_hip_map *m, int32_t origin[3], int64_t *moves) {
  return guarded([&] {
    need(m && origin, "null argument");
    need(m->hash != nullptr, "fiesta_hip_hash_window: not a hash-block map");
    m->hash->window_origin(origin);
    if (moves) *moves = m->hash->window_moves();
  });
}
int fiesta_hip_hash_recentre(fiesta_hip_map *m, const int32_t centre[3]) {
  return guarded([&] {
    need(m && centre, "null argument");
    need(m->hash != nullptr, "fiesta_hip_hash_recentre: not a hash-block map");
    m->hash->recentre(centre);
  });
}

int fiesta_hip_set_prob_params(fiesta_hip_map *m, double p_hit, double p_miss, double p_min, double p_max,
                               double p_occ) {
  return guarded([&] {
    need(m != nullptr, "null map handle");
    on_store(m, [&](auto &s) { s.set_prob_params(p_hit, p_miss, p_min, p_max, p_occ); });
  });
}
int fiesta_hip_set_update_range(fiesta_hip_map *m, const double mn[3], const double mx[3], int new_vec) {
  return guarded([&] {
    need(m && mn && mx, "null argument");
    on_store(m, [&](auto &s) { s.set_update_range(mn, mx, new_vec != 0); });
  });
}
int fiesta_hip_set_original_range(fiesta_hip_map *m) {
  return guarded([&] {
    need(m != nullptr, "null map handle");
    on_store(m, [&](auto &s) { s.set_original_range(); });
  });
}

int fiesta_hip_set_update_engine(fiesta_hip_map *m, int32_t engine) {
  return guarded([&] {
    need(m != nullptr, "null map handle");
    need(engine >= 0 && engine <= 6, "unknown update_engine");
    // (no transform on a hash-block map: 2, 4, 5 and 6 mean 0 there)
    on_store(m, [&](auto &s) { s.set_update_engine(m->hash && engine > 3 ? 0 : engine); });
  });
}

int fiesta_hip_level_trace(fiesta_hip_map *m, uint32_t out[48], int32_t *n_levels) {
  return guarded([&] {
    need(m && out && n_levels, "bad argument");
    *n_levels = on_store(m, [&](auto &s) { return s.level_trace(out); });
  });
}

int fiesta_hip_level_tuning(fiesta_hip_map *m, int32_t grid_groups, int64_t spin_limit) {
  return guarded([&] {
    need(m != nullptr, "null map handle");
    need(grid_groups <= 32, "at most 32 work-groups (the CUs of one XCD)");
    need(spin_limit <= 0xFFFFFFFFll, "spin_limit does not fit 32 bits");
    on_store(m, [&](auto &s) { s.level_tuning(grid_groups, spin_limit); });
  });
}

int fiesta_hip_set_occupancy_vox(fiesta_hip_map *m, const int32_t *vox, const int32_t *occ, int64_t n, int32_t *ret) {
  return guarded([&] {
    need(m && (n == 0 || (vox && occ)) && n >= 0, "bad argument");
    on_store(m, [&](auto &s) { s.observe_vox(vox, occ, n, ret, false); });
  });
}
int fiesta_hip_set_occupancy_pos(fiesta_hip_map *m, const double *pos, const int32_t *occ, int64_t n, int32_t *ret) {
  return guarded([&] {
    need(m && (n == 0 || (pos && occ)) && n >= 0, "bad argument");
    on_store(m, [&](auto &s) { s.observe_pos(pos, occ, n, ret); });
  });
}
int fiesta_hip_set_occupancy_vox_dev(fiesta_hip_map *m, const int32_t *vox_dev, const int32_t *occ_dev, int64_t n) {
  return guarded([&] {
    need(m && (n == 0 || (vox_dev && occ_dev)) && n >= 0, "bad argument");
    on_store(m, [&](auto &s) { s.observe_vox(vox_dev, occ_dev, n, nullptr, true); });
  });
}

int fiesta_hip_set_occupancy_box(fiesta_hip_map *m, const int32_t lo[3], const int32_t hi[3], int32_t occ) {
  return guarded([&] {
    need(m && lo && hi && (occ == 0 || occ == 1), "bad argument");
    on_store(m, [&](auto &s) { s.observe_box(lo, hi, occ); });
  });
}

int fiesta_hip_raycast_frame(fiesta_hip_map *m, const float *points, int64_t n, const double T[16],
                             const double origin[3], const fiesta_hip_raycast_params *p) {
  return guarded([&] {
    need(m && (n == 0 || points) && T && origin && p && n >= 0, "bad argument");
    on_store(m, [&](auto &s) { s.raycast_frame(points, n, T, origin, p, false); });
  });
}
int fiesta_hip_raycast_frame_dev(fiesta_hip_map *m, const float *points_dev, int64_t n, const double T[16],
                                 const double origin[3], const fiesta_hip_raycast_params *p) {
  return guarded([&] {
    need(m && (n == 0 || points_dev) && T && origin && p && n >= 0, "bad argument");
    on_store(m, [&](auto &s) { s.raycast_frame(points_dev, n, T, origin, p, true); });
  });
}
int fiesta_hip_raycast_depth(fiesta_hip_map *m, const uint16_t *depth, int32_t rows, int32_t cols, double fx,
                             double fy, double cx, double cy, const double T[16], const double origin[3],
                             const fiesta_hip_raycast_params *p) {
  return guarded([&] {
    need(m && depth && rows > 0 && cols > 0 && T && origin && p, "bad argument");
    on_store(m, [&](auto &s) { s.raycast_depth(depth, rows, cols, fx, fy, cx, cy, T, origin, p); });
  });
}
int fiesta_hip_raycast_depth_filtered(fiesta_hip_map *m, const uint16_t *depth, int32_t rows, int32_t cols, double fx, double fy,
                                      double cx, double cy, const double T[16], const double origin[3],
                                      const fiesta_hip_raycast_params *p, const fiesta_hip_depth_filter *f) {
  return guarded([&] {
    need(m && depth && rows > 0 && cols > 0 && T && origin && p && f, "bad argument");
    on_store(m, [&](auto &s) { s.raycast_depth(depth, rows, cols, fx, fy, cx, cy, T, origin, p, f); });
  });
}
int fiesta_hip_depth_conversion(fiesta_hip_map *m, const uint16_t *depth, int32_t rows, int32_t cols, double fx, double fy,
                                double cx, double cy, const fiesta_hip_depth_filter *f, float *points_out, int64_t *n_valid) {
  return guarded([&] {
    need(depth && rows > 0 && cols > 0 && points_out, "bad argument");
    const int64_t n = dense(m, "depth_conversion").depth_conversion(depth, rows, cols, fx, fy, cx, cy, f, points_out);
    if (n_valid) *n_valid = n;
  });
}
int fiesta_hip_raycast_single(const double start[3], const double end[3], const double minv[3],
                              const double maxv[3], double *out, int32_t cap, int32_t *n_out, int32_t device) {
  return guarded([&] {
    need(start && end && minv && maxv && n_out && (cap == 0 || out), "bad argument");
    fiesta::raycast_single(start, end, minv, maxv, out, cap, n_out, device);
  });
}

int fiesta_hip_check_update(fiesta_hip_map *m, int32_t *out) {
  return guarded([&] {
    need(m && out, "null argument");
    *out = on_store(m, [&](auto &s) { return s.check_update(); }) ? 1 : 0;
  });
}
int fiesta_hip_update_occupancy(fiesta_hip_map *m, int32_t global_map, int64_t *n_insert, int64_t *n_delete,
                                int32_t *any) {
  return guarded([&] {
    need(m != nullptr, "null map handle");
    const bool r = on_store(m, [&](auto &s) { return s.update_occupancy(global_map != 0, n_insert, n_delete); });
    if (any) *any = r ? 1 : 0;
  });
}
int fiesta_hip_update_esdf(fiesta_hip_map *m, fiesta_hip_stats *stats) {
  return guarded([&] {
    need(m != nullptr, "null map handle");
    on_store(m, [&](auto &s) { s.update_esdf(stats); });
    if (stats && m->dense) stats->path_notes = (int64_t)m->dense->path_notes();
  });
}

int fiesta_hip_get_distance_vox(fiesta_hip_map *m, const int32_t *vox, int64_t n, double *out) {
  return guarded([&] {
    need(m && (n == 0 || (vox && out)) && n >= 0, "bad argument");
    on_store(m, [&](auto &s) { s.get_distance_vox(vox, n, out); });
  });
}
int fiesta_hip_get_distance_pos(fiesta_hip_map *m, const double *pos, int64_t n, double *out) {
  return guarded([&] {
    need(m && (n == 0 || (pos && out)) && n >= 0, "bad argument");
    on_store(m, [&](auto &s) { s.get_distance_pos(pos, n, out); });
  });
}
int fiesta_hip_get_dist_grad(fiesta_hip_map *m, const double *pos, int64_t n, double *dist, double *grad) {
  return guarded([&] {
    need(m && (n == 0 || (pos && dist)) && n >= 0, "bad argument");
    if (m->dense)  // (the array store's member serves the _dev variant too)
      m->dense->get_dist_grad(pos, n, dist, grad, false);
    else
      m->hash->get_dist_grad(pos, n, dist, grad);
  });
}
int fiesta_hip_get_dist_grad_dev(fiesta_hip_map *m, const double *pos_dev, int64_t n, double *dist_dev,
                                 double *grad_dev) {
  return guarded([&] {
    need(m && (n == 0 || (pos_dev && dist_dev)) && n >= 0, "bad argument");
    dense(m, "get_dist_grad_dev").get_dist_grad(pos_dev, n, dist_dev, grad_dev, true);
  });
}
int fiesta_hip_path_clearance(fiesta_hip_map *m, const double *w, int64_t n_wp, const int64_t *off, int64_t n_paths, double step,
                              double margin, const fiesta_hip_path_result *r) {
  return guarded([&] { path_clearance(m, {w, n_wp, off, n_paths, step, margin, r, false}); });
}
int fiesta_hip_path_clearance_dev(fiesta_hip_map *m, const double *w_dev, int64_t n_wp, const int64_t *off_dev, int64_t n_paths,
                                  double step, double margin, const fiesta_hip_path_result *r) {
  return guarded([&] { path_clearance(m, {w_dev, n_wp, off_dev, n_paths, step, margin, r, true}); });
}
int fiesta_hip_path_cost(fiesta_hip_map *m, const double *w, int64_t n_wp, const int64_t *off, int64_t n_paths, double step, double margin,
                         const fiesta_hip_path_cost_result *r) {
  return guarded([&] { path_cost(m, {w, n_wp, off, n_paths, step, margin, r, false}); });
}
int fiesta_hip_path_cost_dev(fiesta_hip_map *m, const double *w_dev, int64_t n_wp, const int64_t *off_dev, int64_t n_paths, double step,
                             double margin, const fiesta_hip_path_cost_result *r) {
  return guarded([&] { path_cost(m, {w_dev, n_wp, off_dev, n_paths, step, margin, r, true}); });
}
int fiesta_hip_path_refine(fiesta_hip_map *m, const double *w, int64_t n_wp, const int64_t *off, int64_t n_paths, const double *bounds,
                           const fiesta_hip_refine_params *par, const fiesta_hip_refine_result *r) {
  return guarded([&] { path_refine(m, {w, n_wp, off, n_paths, bounds, par, r, false}); });
}
int fiesta_hip_path_refine_dev(fiesta_hip_map *m, const double *w_dev, int64_t n_wp, const int64_t *off_dev, int64_t n_paths,
                               const double *bounds_dev, const fiesta_hip_refine_params *par, const fiesta_hip_refine_result *r) {
  return guarded([&] { path_refine(m, {w_dev, n_wp, off_dev, n_paths, bounds_dev, par, r, true}); });
}
int fiesta_hip_path_timing(fiesta_hip_map *m, const double *w, int64_t n_wp, const int64_t *off, int64_t n_paths,
                           const fiesta_hip_timing_params *par, const fiesta_hip_path_timing_result *r) {
  return guarded([&] { path_timing(m, {w, n_wp, off, n_paths, par, r, false}); });
}
int fiesta_hip_path_timing_dev(fiesta_hip_map *m, const double *w_dev, int64_t n_wp, const int64_t *off_dev, int64_t n_paths,
                               const fiesta_hip_timing_params *par, const fiesta_hip_path_timing_result *r) {
  return guarded([&] { path_timing(m, {w_dev, n_wp, off_dev, n_paths, par, r, true}); });
}
int fiesta_hip_corridor_bounds(fiesta_hip_map *m, const int32_t *w, int64_t n_wp, const int64_t *off, int64_t n_paths, const int64_t *box_off,
                               const int32_t *boxes, const double *boxes_pos, const int32_t *entry, const int32_t *status, int64_t n_boxes,
                               double inset, int32_t flags, const fiesta_hip_bounds_result *r) {
  return guarded([&] { corridor_bounds(m, {w, n_wp, off, n_paths, box_off, boxes, boxes_pos, entry, status, n_boxes, inset, flags, r, false}); });
}
int fiesta_hip_corridor_bounds_dev(fiesta_hip_map *m, const int32_t *w_dev, int64_t n_wp, const int64_t *off_dev, int64_t n_paths,
                                   const int64_t *box_off_dev, const int32_t *boxes_dev, const double *boxes_pos_dev, const int32_t *entry_dev,
                                   const int32_t *status_dev, int64_t n_boxes, double inset, int32_t flags, const fiesta_hip_bounds_result *r) {
  return guarded([&] {
    corridor_bounds(m, {w_dev, n_wp, off_dev, n_paths, box_off_dev, boxes_dev, boxes_pos_dev, entry_dev, status_dev, n_boxes, inset, flags, r, true});
  });
}
int fiesta_hip_host_cache_fetches(fiesta_hip_map *m, int64_t *fetches) {
  return guarded([&] {
    need(m && fetches, "bad argument");
    *fetches = on_store(m, [&](auto &s) { return s.host_brick_fetches(); });
  });
}
int fiesta_hip_get_occupancy_vox(fiesta_hip_map *m, const int32_t *vox, int64_t n, int32_t *out) {
  return guarded([&] {
    need(m && (n == 0 || (vox && out)) && n >= 0, "bad argument");
    on_store(m, [&](auto &s) { s.get_occupancy_vox(vox, n, out); });
  });
}
int fiesta_hip_get_occupancy_pos(fiesta_hip_map *m, const double *pos, int64_t n, int32_t *out) {
  return guarded([&] {
    need(m && (n == 0 || (pos && out)) && n >= 0, "bad argument");
    on_store(m, [&](auto &s) { s.get_occupancy_pos(pos, n, out); });
  });
}

int fiesta_hip_download_field(fiesta_hip_map *m, int32_t *d2, int32_t *coc, uint8_t *occ, double *logodds) {
  return guarded([&] { dense(m, "download_field").download_field(d2, coc, occ, logodds); });
}
int fiesta_hip_download_counts(fiesta_hip_map *m, int32_t *num_hit, int32_t *num_miss) {
  return guarded([&] {
    need(m != nullptr, "null map");
    on_store(m, [&](auto &s) { s.download_counts(num_hit, num_miss); });
  });
}
int fiesta_hip_count_no_obstacle(fiesta_hip_map *m, int64_t *n_out) {
  return guarded([&] {
    need(m && n_out, "null argument");
    *n_out = dense(m, "count_no_obstacle").count_no_obstacle();
  });
}
int fiesta_hip_get_occupied_voxels(fiesta_hip_map *m, int32_t *vox, int64_t capacity, int64_t *n_out) {
  return guarded([&] {
    need(n_out != nullptr && capacity >= 0, "bad argument");
    *n_out = dense(m, "get_occupied_voxels").occupied_voxels(vox, capacity);
  });
}
int fiesta_hip_body_query(fiesta_hip_map *m, const double *spheres, int32_t n_spheres, const double *poses, int64_t n_poses, double margin,
                          const fiesta_hip_body_result *result) {
  return guarded([&] { body_query(m, {spheres, n_spheres, poses, n_poses, margin, result, false}); });
}
int fiesta_hip_body_query_dev(fiesta_hip_map *m, const double *spheres, int32_t n_spheres, const double *poses_dev, int64_t n_poses, double margin,
                              const fiesta_hip_body_result *result) {
  return guarded([&] { body_query(m, {spheres, n_spheres, poses_dev, n_poses, margin, result, true}); });
}
int fiesta_hip_articulated_query(fiesta_hip_map *m, const double *spheres, const int32_t *sphere_frame, int32_t n_spheres, int32_t n_frames,
                                 const double *frame_poses, int64_t n_configs, double margin, const fiesta_hip_articulated_result *result) {
  return guarded([&] { articulated_query(m, {spheres, sphere_frame, n_spheres, n_frames, frame_poses, n_configs, margin, result, false}); });
}
int fiesta_hip_articulated_query_dev(fiesta_hip_map *m, const double *spheres, const int32_t *sphere_frame, int32_t n_spheres, int32_t n_frames,
                                     const double *frame_poses_dev, int64_t n_configs, double margin,
                                     const fiesta_hip_articulated_result *result) {
  return guarded([&] { articulated_query(m, {spheres, sphere_frame, n_spheres, n_frames, frame_poses_dev, n_configs, margin, result, true}); });
}
int fiesta_hip_body_sweep(fiesta_hip_map *m, const double *spheres, int32_t n_spheres, const double *poses, int64_t n_poses,
                          const int64_t *offsets, int64_t n_paths, double step, double margin, const fiesta_hip_sweep_result *result) {
  return guarded([&] { body_sweep(m, {spheres, n_spheres, poses, n_poses, offsets, n_paths, step, margin, result, false}); });
}
int fiesta_hip_body_sweep_dev(fiesta_hip_map *m, const double *spheres, int32_t n_spheres, const double *poses_dev, int64_t n_poses,
                              const int64_t *offsets_dev, int64_t n_paths, double step, double margin,
                              const fiesta_hip_sweep_result *result) {
  return guarded([&] { body_sweep(m, {spheres, n_spheres, poses_dev, n_poses, offsets_dev, n_paths, step, margin, result, true}); });
}
int fiesta_hip_get_frontier_voxels(fiesta_hip_map *m, const int32_t lo[3], const int32_t hi[3], double min_clearance, int32_t *vox,
                                   uint8_t *mask, int64_t capacity, int64_t *n_out) {
  return guarded([&] { *n_out = frontier_voxels(m, {lo, hi, min_clearance, vox, mask, capacity, nullptr, false}, n_out); });
}
int fiesta_hip_get_frontier_voxels_dev(fiesta_hip_map *m, const int32_t lo[3], const int32_t hi[3], double min_clearance, int32_t *vox_dev,
                                       uint8_t *mask_dev, int64_t capacity, unsigned long long *n_out_dev) {
  return guarded([&] { frontier_voxels(m, {lo, hi, min_clearance, vox_dev, mask_dev, capacity, n_out_dev, true}, n_out_dev); });
}
int fiesta_hip_get_skeleton_voxels(fiesta_hip_map *m, const int32_t lo[3], const int32_t hi[3], int32_t min_sep2, double min_clearance,
                                   int64_t capacity, const fiesta_hip_skeleton_result *result, int64_t *n_out) {
  return guarded([&] { *n_out = skeleton_voxels(m, {lo, hi, min_sep2, min_clearance, capacity, result, nullptr, false}, n_out); });
}
int fiesta_hip_get_skeleton_voxels_dev(fiesta_hip_map *m, const int32_t lo[3], const int32_t hi[3], int32_t min_sep2, double min_clearance,
                                       int64_t capacity, const fiesta_hip_skeleton_result *result, unsigned long long *n_out_dev) {
  return guarded([&] { skeleton_voxels(m, {lo, hi, min_sep2, min_clearance, capacity, result, n_out_dev, true}, n_out_dev); });
}
int fiesta_hip_ray_query(fiesta_hip_map *m, const double *start, const double *end, int64_t n, int32_t stop_mask,
                         const fiesta_hip_ray_result *r) {
  return guarded([&] { ray_query(m, {start, end, n, stop_mask, r, false}); });
}
int fiesta_hip_ray_query_dev(fiesta_hip_map *m, const double *start_dev, const double *end_dev, int64_t n, int32_t stop_mask,
                             const fiesta_hip_ray_result *r) {
  return guarded([&] { ray_query(m, {start_dev, end_dev, n, stop_mask, r, true}); });
}
int fiesta_hip_reach_field(fiesta_hip_map *m, const int32_t lo[3], const int32_t hi[3], const int32_t *seeds, int64_t n_seeds,
                           const int32_t *targets, int64_t n_targets, double min_clearance, int32_t connectivity, int32_t flags,
                           const fiesta_hip_reach_result *result, fiesta_hip_reach_info *info) {
  return guarded([&] { reach_field(m, {lo, hi, seeds, n_seeds, targets, n_targets, min_clearance, connectivity, flags, result, info, false}); });
}
int fiesta_hip_reach_field_dev(fiesta_hip_map *m, const int32_t lo[3], const int32_t hi[3], const int32_t *seeds_dev, int64_t n_seeds,
                               const int32_t *targets_dev, int64_t n_targets, double min_clearance, int32_t connectivity, int32_t flags,
                               const fiesta_hip_reach_result *result, fiesta_hip_reach_info *info) {
  return guarded([&] { reach_field(m, {lo, hi, seeds_dev, n_seeds, targets_dev, n_targets, min_clearance, connectivity, flags, result, info, true}); });
}
int fiesta_hip_reach_matrix(fiesta_hip_map *m, const int32_t lo[3], const int32_t hi[3], const int32_t *sources, int64_t n_sources,
                            const int32_t *targets, int64_t n_targets, double min_clearance, int32_t connectivity, int32_t flags,
                            int32_t max_fields, const fiesta_hip_reach_matrix_result *result, fiesta_hip_reach_matrix_info *info) {
  return guarded(
      [&] { reach_matrix(m, {lo, hi, sources, n_sources, targets, n_targets, min_clearance, connectivity, flags, max_fields, result, info, false}); });
}
int fiesta_hip_reach_matrix_dev(fiesta_hip_map *m, const int32_t lo[3], const int32_t hi[3], const int32_t *sources_dev, int64_t n_sources,
                                const int32_t *targets_dev, int64_t n_targets, double min_clearance, int32_t connectivity, int32_t flags,
                                int32_t max_fields, const fiesta_hip_reach_matrix_result *result, fiesta_hip_reach_matrix_info *info) {
  return guarded([&] {
    reach_matrix(m, {lo, hi, sources_dev, n_sources, targets_dev, n_targets, min_clearance, connectivity, flags, max_fields, result, info, true});
  });
}
int fiesta_hip_site_tour(fiesta_hip_map *m, const int32_t *cost, int32_t n, int64_t ld, int32_t start, int32_t flags, int32_t restarts,
                         uint64_t seed, int32_t max_moves, const fiesta_hip_tour_result *result, fiesta_hip_tour_info *info) {
  return guarded([&] { site_tour(m, {cost, n, ld, start, flags, restarts, seed, max_moves, result, info, false}); });
}
int fiesta_hip_site_tour_dev(fiesta_hip_map *m, const int32_t *cost_dev, int32_t n, int64_t ld, int32_t start, int32_t flags, int32_t restarts,
                             uint64_t seed, int32_t max_moves, const fiesta_hip_tour_result *result, fiesta_hip_tour_info *info) {
  return guarded([&] { site_tour(m, {cost_dev, n, ld, start, flags, restarts, seed, max_moves, result, info, true}); });
}
int fiesta_hip_reach_paths(fiesta_hip_map *m, const int32_t *cost, const int32_t box_lo[3], const int32_t box_hi[3], const int32_t *targets,
                           int64_t n_targets, int32_t connectivity, int32_t flags, int32_t max_span, int64_t capacity,
                           const fiesta_hip_reach_paths_result *result) {
  return guarded([&] { reach_paths(m, {cost, box_lo, box_hi, targets, n_targets, connectivity, flags, max_span, capacity, result, false}); });
}
int fiesta_hip_reach_paths_dev(fiesta_hip_map *m, const int32_t *cost_dev, const int32_t box_lo[3], const int32_t box_hi[3],
                               const int32_t *targets_dev, int64_t n_targets, int32_t connectivity, int32_t flags, int32_t max_span,
                               int64_t capacity, const fiesta_hip_reach_paths_result *result) {
  return guarded([&] { reach_paths(m, {cost_dev, box_lo, box_hi, targets_dev, n_targets, connectivity, flags, max_span, capacity, result, true}); });
}
int fiesta_hip_leg_paths(fiesta_hip_map *m, const int32_t *from, const int32_t *to, const int32_t *to_vox, int64_t n_legs, int32_t flags,
                         int32_t max_span, int64_t capacity, const fiesta_hip_leg_paths_result *result, fiesta_hip_leg_paths_info *info) {
  return guarded([&] { leg_paths(m, {from, to, to_vox, n_legs, flags, max_span, capacity, result, info, false}); });
}
int fiesta_hip_leg_paths_dev(fiesta_hip_map *m, const int32_t *from_dev, const int32_t *to_dev, const int32_t *to_vox_dev, int64_t n_legs,
                             int32_t flags, int32_t max_span, int64_t capacity, const fiesta_hip_leg_paths_result *result,
                             fiesta_hip_leg_paths_info *info) {
  return guarded([&] { leg_paths(m, {from_dev, to_dev, to_vox_dev, n_legs, flags, max_span, capacity, result, info, true}); });
}
int fiesta_hip_free_boxes(fiesta_hip_map *m, const int32_t lo[3], const int32_t hi[3], const int32_t *seeds, int64_t n, double min_clearance,
                          int32_t max_grow, int32_t flags, const fiesta_hip_free_boxes_result *result) {
  return guarded([&] { corridor(m, {false, lo, hi, seeds, n, nullptr, 0, min_clearance, max_grow, flags, 0, result, nullptr, false}); });
}
int fiesta_hip_free_boxes_dev(fiesta_hip_map *m, const int32_t lo[3], const int32_t hi[3], const int32_t *seeds_dev, int64_t n,
                              double min_clearance, int32_t max_grow, int32_t flags, const fiesta_hip_free_boxes_result *result) {
  return guarded([&] { corridor(m, {false, lo, hi, seeds_dev, n, nullptr, 0, min_clearance, max_grow, flags, 0, result, nullptr, true}); });
}
int fiesta_hip_path_corridor(fiesta_hip_map *m, const int32_t lo[3], const int32_t hi[3], const int32_t *waypoints_vox, int64_t n_waypoints,
                             const int64_t *offsets, int64_t n_paths, double min_clearance, int32_t max_grow, int32_t flags,
                             int64_t capacity, const fiesta_hip_corridor_result *result) {
  return guarded([&] {
    corridor(m, {true, lo, hi, waypoints_vox, n_waypoints, offsets, n_paths, min_clearance, max_grow, flags, capacity, nullptr, result, false});
  });
}
int fiesta_hip_path_corridor_dev(fiesta_hip_map *m, const int32_t lo[3], const int32_t hi[3], const int32_t *waypoints_vox_dev,
                                 int64_t n_waypoints, const int64_t *offsets_dev, int64_t n_paths, double min_clearance, int32_t max_grow,
                                 int32_t flags, int64_t capacity, const fiesta_hip_corridor_result *result) {
  return guarded([&] {
    corridor(m, {true, lo, hi, waypoints_vox_dev, n_waypoints, offsets_dev, n_paths, min_clearance, max_grow, flags, capacity, nullptr, result, true});
  });
}
int fiesta_hip_split_clusters(fiesta_hip_map *m, const int32_t *vox, const uint8_t *mask, const int32_t *key, int64_t n, const int64_t *offsets,
                              const int64_t *members, int64_t n_clusters, int64_t n_members, int32_t max_size, int32_t max_extent,
                              int32_t max_depth, int64_t part_capacity, const fiesta_hip_split_result *result, fiesta_hip_split_info *info) {
  return guarded([&] {
    split_clusters(m, {vox, mask, key, n, offsets, members, n_clusters, nullptr, n_members, max_size, max_extent, max_depth, part_capacity, result, info, false});
  });
}
int fiesta_hip_split_clusters_dev(fiesta_hip_map *m, const int32_t *vox_dev, const uint8_t *mask_dev, const int32_t *key_dev, int64_t n,
                                  const int64_t *offsets_dev, const int64_t *members_dev, int64_t n_clusters, const int64_t *n_clusters_dev,
                                  int64_t n_members, int32_t max_size, int32_t max_extent, int32_t max_depth, int64_t part_capacity,
                                  const fiesta_hip_split_result *result, fiesta_hip_split_info *info_dev) {
  return guarded([&] {
    split_clusters(m, {vox_dev, mask_dev, key_dev, n, offsets_dev, members_dev, n_clusters, n_clusters_dev, n_members, max_size, max_extent, max_depth,
                       part_capacity, result, info_dev, true});
  });
}
int fiesta_hip_cluster_voxels(fiesta_hip_map *m, const int32_t *vox, const uint8_t *mask, const int32_t *key, int64_t n, int32_t connectivity,
                              int32_t min_size, int64_t cluster_capacity, int64_t member_capacity, const fiesta_hip_cluster_result *result,
                              fiesta_hip_cluster_info *info) {
  return guarded([&] { cluster_voxels(m, {vox, mask, key, n, nullptr, connectivity, min_size, cluster_capacity, member_capacity, result, info, false}); });
}
int fiesta_hip_cluster_voxels_dev(fiesta_hip_map *m, const int32_t *vox_dev, const uint8_t *mask_dev, const int32_t *key_dev, int64_t n,
                                  const unsigned long long *n_dev, int32_t connectivity, int32_t min_size, int64_t cluster_capacity,
                                  int64_t member_capacity, const fiesta_hip_cluster_result *result, fiesta_hip_cluster_info *info_dev) {
  return guarded([&] {
    cluster_voxels(m, {vox_dev, mask_dev, key_dev, n, n_dev, connectivity, min_size, cluster_capacity, member_capacity, result, info_dev, true});
  });
}
int fiesta_hip_view_coverage(fiesta_hip_map *m, const int32_t *vox, int64_t n, const int64_t *offsets, const int64_t *members, int64_t n_groups,
                             int64_t n_members, const fiesta_hip_view_set *views, const fiesta_hip_view_sensor *sensor,
                             const fiesta_hip_view_result *result, fiesta_hip_view_info *info) {
  return guarded([&] { view_coverage(m, {vox, n, offsets, members, n_groups, nullptr, n_members, views, sensor, result, info, false}); });
}
int fiesta_hip_view_coverage_dev(fiesta_hip_map *m, const int32_t *vox_dev, int64_t n, const int64_t *offsets_dev, const int64_t *members_dev,
                                 int64_t n_groups, const int64_t *n_groups_dev, int64_t n_members, const fiesta_hip_view_set *views,
                                 const fiesta_hip_view_sensor *sensor, const fiesta_hip_view_result *result, fiesta_hip_view_info *info_dev) {
  return guarded([&] {
    view_coverage(m, {vox_dev, n, offsets_dev, members_dev, n_groups, n_groups_dev, n_members, views, sensor, result, info_dev, true});
  });
}
int fiesta_hip_get_slice(fiesta_hip_map *m, int32_t z_vox, double *out) {
  return guarded([&] {
    need(out != nullptr, "null argument");
    dense(m, "get_slice").slice_distances(z_vox, out);
  });
}
int fiesta_hip_save(fiesta_hip_map *m, const char *path) {
  return guarded([&] {
    need(m && path, "null argument");
    on_store(m, [&](auto &s) { s.checkpoint(path, true); });
  });
}
int fiesta_hip_load(fiesta_hip_map *m, const char *path) {
  return guarded([&] {
    need(m && path, "null argument");
    on_store(m, [&](auto &s) { s.checkpoint(path, false); });
  });
}
int fiesta_hip_get_point_cloud(fiesta_hip_map *m, int32_t vis_lower_bound, int32_t vis_upper_bound, float *xyz,
                               int64_t capacity, int64_t *n_out) {
  return guarded([&] {
    need(m && n_out && capacity >= 0, "bad argument");
    *n_out = on_store(m, [&](auto &s) { return s.point_cloud(vis_lower_bound, vis_upper_bound, xyz, capacity); });
  });
}
int fiesta_hip_get_slice_marker(fiesta_hip_map *m, int32_t slice, double max_dist, double *xyz, float *rgba,
                                int64_t capacity, int64_t *n_out) {
  return guarded([&] {
    need(m && n_out && capacity >= 0, "bad argument");
    *n_out = on_store(m, [&](auto &s) { return s.slice_marker(slice, max_dist, xyz, rgba, capacity); });
  });
}
int fiesta_hip_download_hash(fiesta_hip_map *m, int64_t *n_out, int32_t *vox, int32_t *d2, int32_t *coc,
                             uint8_t *occ) {
  return guarded([&] {
    need(m && n_out, "null argument");
    if (!m->hash) throw Error(FIESTA_HIP_ERR_INVALID, "download_hash: only available on hash-mode maps");
    *n_out = m->hash->download(vox, d2, coc, occ);
  });
}

int fiesta_hip_snapshot_save(fiesta_hip_map *m, int32_t slot) {
  return guarded([&] {
    need(m != nullptr, "null map");
    if (m->dense) return m->dense->snapshot_save(slot);
    // hash-block maps keep ONE copy of the state words, enough for the "updated voxels" unit (no restore)
    need(slot == 0, "hash-mode maps have snapshot slot 0 only");
    m->hash->snapshot_save();
  });
}
int fiesta_hip_snapshot_restore(fiesta_hip_map *m, int32_t slot) {
  return guarded([&] { dense(m, "snapshot_restore").snapshot_restore(slot); });
}
int fiesta_hip_snapshot_count_updated(fiesta_hip_map *m, int32_t slot, int64_t *updated) {
  return guarded([&] {
    need(updated != nullptr, "null argument");
    need(m != nullptr, "null map");
    if (!m->dense) need(slot == 0, "hash-mode maps have snapshot slot 0 only");
    *updated = m->dense ? m->dense->snapshot_count_updated(slot) : m->hash->snapshot_count_updated();
  });
}

int fiesta_hip_shard_info_get(fiesta_hip_map *m, fiesta_hip_shard_info *out) {
  return guarded([&] {
    need(out != nullptr, "null argument");
    const fiesta::Geom &g = dense(m, "shard_info").geom();
    out->local_dims[0] = g.nx, out->local_dims[1] = g.ny, out->local_dims[2] = g.nz;
    out->local_origin[0] = g.gx0, out->local_origin[1] = g.gy0, out->local_origin[2] = g.gz0;
    out->owned_lo[0] = g.ox0, out->owned_lo[1] = g.oy0, out->owned_lo[2] = g.oz0;
    out->owned_hi[0] = g.ox1, out->owned_hi[1] = g.oy1, out->owned_hi[2] = g.oz1;
    out->global_grid[0] = g.GX, out->global_grid[1] = g.GY, out->global_grid[2] = g.GZ;
  });
}
int fiesta_hip_halo_pack_dev(fiesta_hip_map *m, const int32_t lo[3], const int32_t hi[3], uint32_t *out_dev) {
  return guarded([&] {
    need(lo && hi && out_dev, "null argument");
    dense(m, "halo_pack").halo_pack(lo, hi, out_dev);
  });
}
int fiesta_hip_halo_apply_dev(fiesta_hip_map *m, const int32_t lo[3], const int32_t hi[3], const uint32_t *in_dev,
                              int64_t *n_changed) {
  return guarded([&] {
    need(lo && hi && in_dev, "null argument");
    const int64_t k = dense(m, "halo_apply").halo_apply(lo, hi, in_dev);
    if (n_changed) *n_changed = k;
  });
}
int fiesta_hip_export_transitions_dev(fiesta_hip_map *m, uint32_t *out_dev, int64_t capacity, int64_t *n_out) {
  return guarded([&] {
    need(n_out != nullptr, "null argument");
    *n_out = dense(m, "export_transitions").export_transitions(out_dev, capacity);
  });
}
int fiesta_hip_apply_transitions_dev(fiesta_hip_map *m, const uint32_t *entries_dev, int64_t n) {
  return guarded([&] {
    need(n == 0 || entries_dev, "null argument");
    dense(m, "apply_transitions").apply_transitions(entries_dev, n);
  });
}
int fiesta_hip_halo_pack(fiesta_hip_map *m, const int32_t lo[3], const int32_t hi[3], uint32_t *out) {
  return guarded([&] {
    need(lo && hi && out, "null argument");
    DenseMap &d = dense(m, "halo_pack");
    const int64_t n = (int64_t)(hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1);
    need(n > 0, "empty box");
    uint32_t *buf = d.scratch_u32(n);
    d.halo_pack(lo, hi, buf);
    d.copy_to_host(out, buf, n * sizeof(uint32_t));
  });
}
int fiesta_hip_halo_apply(fiesta_hip_map *m, const int32_t lo[3], const int32_t hi[3], const uint32_t *in,
                          int64_t *n_changed) {
  return guarded([&] {
    need(lo && hi && in, "null argument");
    DenseMap &d = dense(m, "halo_apply");
    const int64_t n = (int64_t)(hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1);
    need(n > 0, "empty box");
    uint32_t *buf = d.scratch_u32(n);
    d.copy_to_device(buf, in, n * sizeof(uint32_t));
    const int64_t k = d.halo_apply(lo, hi, buf);
    if (n_changed) *n_changed = k;
  });
}
int fiesta_hip_export_transitions(fiesta_hip_map *m, uint32_t *out, int64_t capacity, int64_t *n_out) {
  return guarded([&] {
    need(n_out != nullptr, "null argument");
    DenseMap &d = dense(m, "export_transitions");
    const int64_t n = d.export_transitions(nullptr, 0);
    *n_out = n;
    if (!out || n == 0) return;
    need(n <= capacity, "transition buffer too small");
    uint32_t *buf = d.scratch_u32(2 * n);
    d.export_transitions(buf, n);
    d.copy_to_host(out, buf, 2 * n * sizeof(uint32_t));
  });
}
int fiesta_hip_apply_transitions(fiesta_hip_map *m, const uint32_t *entries, int64_t n) {
  return guarded([&] {
    need(n == 0 || entries, "null argument");
    if (n == 0) return;
    DenseMap &d = dense(m, "apply_transitions");
    uint32_t *buf = d.scratch_u32(2 * n);
    d.copy_to_device(buf, entries, 2 * n * sizeof(uint32_t));
    d.apply_transitions(buf, n);
  });
}
int fiesta_hip_esdf_seed(fiesta_hip_map *m, fiesta_hip_stats *stats) {
  return guarded([&] { dense(m, "esdf_seed").update_esdf(stats, true); });
}
int fiesta_hip_relax_pending(fiesta_hip_map *m, fiesta_hip_stats *stats, int64_t *pending) {
  return guarded([&] { dense(m, "relax_pending").relax_pending(stats, pending); });
}

int fiesta_hip_rccl_unique_id(uint8_t id[128]) {
  return guarded([&] {
    need(id != nullptr, "null argument");
    fiesta::rccl_unique_id(id);
  });
}
int fiesta_hip_shard_box(const int32_t gg[3], int32_t world, int32_t rank, int32_t lo[3], int32_t size[3]) {
  return guarded([&] {
    need(gg && lo && size, "null argument");
    need(rank >= 0 && rank < world, "rank out of range");
    const int g3[3] = {gg[0], gg[1], gg[2]};
    int l3[3], s3[3];
    fiesta::shard_box(g3, world, rank, l3, s3);
    for (int i = 0; i < 3; ++i) lo[i] = l3[i], size[i] = s3[i];
  });
}
int fiesta_hip_shard_group_create(fiesta_hip_map *const *shards, const int32_t *ranks, int32_t n_local, int32_t world,
                                  const uint8_t *rccl_id, fiesta_hip_shard_group **out) {
  return guarded([&] {
    need(shards && ranks && out && n_local > 0, "null argument");
    *out = nullptr;
    std::vector<DenseMap *> maps;
    std::vector<int> rk;
    for (int i = 0; i < n_local; ++i) {
      maps.push_back(&dense(shards[i], "shard_group_create"));
      rk.push_back(ranks[i]);
    }
    auto *h = new fiesta_hip_shard_group;
    try {
      h->g = new fiesta::ShardGroup(maps, rk, world, rccl_id);
    } catch (...) {
      delete h;
      throw;
    }
    *out = h;
  });
}
int fiesta_hip_shard_group_create_hosted(fiesta_hip_map *shard, int32_t rank, int32_t world, const fiesta_hip_shard_transport *t,
                                         fiesta_hip_shard_group **out) {
  return guarded([&] {
    need(shard && out && t && t->all_gather && t->exchange, "null argument");
    *out = nullptr;
    std::vector<DenseMap *> maps{&dense(shard, "shard_group_create_hosted")};
    std::vector<int> rk{rank};
    auto *h = new fiesta_hip_shard_group;
    try {
      h->g = new fiesta::ShardGroup(maps, rk, world, nullptr, t);
    } catch (...) {
      delete h;
      throw;
    }
    *out = h;
  });
}
int fiesta_hip_shard_group_precheck(fiesta_hip_map *const *shards, const int32_t *ranks, int32_t n_local, int32_t world, int32_t use_rccl) {
  return guarded([&] {
    need(shards && ranks && n_local > 0, "null argument");
    std::vector<DenseMap *> maps;
    std::vector<int> rk;
    for (int i = 0; i < n_local; ++i) {
      maps.push_back(&dense(shards[i], "shard_group_precheck"));
      rk.push_back(ranks[i]);
    }
    fiesta::ShardGroup::precheck(maps, rk, world, use_rccl != 0);
  });
}
int fiesta_hip_shard_group_comm_info(fiesta_hip_shard_group *g, int32_t *nranks, int32_t *rank) {
  return guarded([&] {
    need(g && g->g, "null shard group");
    int n = 0, r = 0;
    g->g->comm_info(&n, &r);
    if (nranks) *nranks = n;
    if (rank) *rank = r;
  });
}
int fiesta_hip_shard_group_destroy(fiesta_hip_shard_group *g) {
  return guarded([&] {
    if (!g) return;
    delete g->g;
    delete g;
  });
}
int fiesta_hip_shard_group_update_occupancy(fiesta_hip_shard_group *g, int32_t global_map, int64_t *n_insert, int64_t *n_delete,
                                            int32_t *any) {
  return guarded([&] {
    need(g && g->g, "null shard group");
    const bool a = g->g->update_occupancy(global_map != 0, n_insert, n_delete);
    if (any) *any = a ? 1 : 0;
  });
}
int fiesta_hip_shard_group_update_esdf(fiesta_hip_shard_group *g, fiesta_hip_stats *stats, int32_t *sweeps, int64_t *entries_sent) {
  return guarded([&] {
    need(g && g->g, "null shard group");
    g->g->update_esdf(stats, sweeps, entries_sent);
  });
}

int fiesta_hip_synchronize(fiesta_hip_map *m) {
  return guarded([&] {
    need(m != nullptr, "null map handle");
    on_store(m, [&](auto &s) { s.synchronize(); });
  });
}

}  // extern "C"
