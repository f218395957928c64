// fiesta_amd/csrc/planner.hip -- the planner calls that read no voxel (planner.hpp), for both stores: the one translation unit that
// includes their kernel headers, so each of their kernels is compiled once.
#include "planner.hpp"

#include "bounds_kernels.hpp"
#include "cluster_kernels.hpp"
#include "leg_path_kernels.hpp"
#include "reach_path_kernels.hpp"
#include "split_kernels.hpp"
#include "tour_kernels.hpp"

namespace fiesta {

static void use_device(const PlannerCtx &ctx) { FIESTA_HIP_CHECK(hipSetDevice(ctx.device)); }

void reach_paths(const PlannerCtx &ctx, const ReachPathArgs &a) { use_device(ctx), reach_paths_run(ctx.stream, ctx.S, ctx.res, ctx.org, a); }
void leg_paths(const PlannerCtx &ctx, const LegPathArgs &a) { use_device(ctx), leg_paths_run(ctx.stream, ctx.S, ctx.res, ctx.org, a); }
void cluster_voxels(const PlannerCtx &ctx, const ClusterArgs &a) { use_device(ctx), cluster_voxels_run(ctx.stream, ctx.S, ctx.res, ctx.org, a); }
void split_clusters(const PlannerCtx &ctx, const SplitArgs &a) { use_device(ctx), split_clusters_run(ctx.stream, ctx.S, ctx.res, ctx.org, a); }
void corridor_bounds(const PlannerCtx &ctx, const CorridorBoundsArgs &a) {
  if (a.n_paths <= 0) return;
  use_device(ctx), corridor_bounds_run(ctx.stream, ctx.S, a);
}
void site_tour(const PlannerCtx &ctx, const TourArgs &a) { use_device(ctx), site_tour_run(ctx.stream, ctx.S, a); }

void reach_path_scan(hipStream_t st, int64_t *offsets, int64_t n) {
  hipLaunchKernelGGL(k_reach_path_scan, dim3(1), dim3(256), 0, st, offsets, n);
}

}  // namespace fiesta
