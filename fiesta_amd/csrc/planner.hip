// fiesta_amd/csrc/planner.hip -- the planner calls (planner.hpp), for both stores: the one translation unit that includes their kernel
// headers, so each kernel is compiled once.  The calls that read voxels are templates over the store's view, instantiated for both.
#include "planner.hpp"

#include "dense_read.hpp"
#include "hash_read.hpp"
#include "articulated_kernels.hpp"
#include "body_kernels.hpp"
#include "bounds_kernels.hpp"
#include "cluster_kernels.hpp"
#include "corridor_kernels.hpp"
#include "frontier_kernels.hpp"
#include "leg_path_kernels.hpp"
#include "path_cost_kernels.hpp"
#include "path_kernels.hpp"
#include "ray_query_kernels.hpp"
#include "reach_kernels.hpp"
#include "reach_matrix_kernels.hpp"
#include "reach_path_kernels.hpp"
#include "refine_kernels.hpp"
#include "skeleton_kernels.hpp"
#include "split_kernels.hpp"
#include "sweep_kernels.hpp"
#include "timing_kernels.hpp"
#include "tour_kernels.hpp"
#include "view_kernels.hpp"

namespace fiesta {

static void use_device(const PlannerCtx &ctx) { FIESTA_HIP_CHECK(hipSetDevice(ctx.device)); }

// ---- the calls that read voxels ---------------------------------------------------------------------------------------------------
// a host batch of at most kHostPathSamples samples is answered from the store's host brick cache
template <class R>
static bool path_on_host(const PathArgs<R> &a) {
  return !a.dev && path_host_samples(a.w, a.off, a.n_paths, a.step, kHostPathSamples) <= kHostPathSamples;
}
template <class View, class HostEval>
void path_clearance(const PlannerCtx &ctx, const View &v, HostEval host, const PathClearanceArgs &a) {
  if (a.n_paths <= 0) return;
  if (path_on_host(a)) return path_host(host, a.w, a.off, a.n_paths, a.step, a.margin, *a.res);
  use_device(ctx), path_clearance_run(ctx.stream, ctx.S, v.path_eval(), a);
}
template <class View, class HostEval>
void path_cost(const PlannerCtx &ctx, const View &v, HostEval host, const PathCostArgs &a) {
  if (a.n_paths <= 0) return;
  if (path_on_host(a)) return path_cost_host(host, a.w, a.n_wp, a.off, a.n_paths, a.step, a.margin, *a.res);
  use_device(ctx), path_cost_run(ctx.stream, ctx.S, v.path_eval(), a);
}
template <class View>
void path_refine(const PlannerCtx &ctx, const View &v, const PathRefineArgs &a) {
  if (a.n_paths <= 0) return;
  use_device(ctx), path_refine_run(ctx.stream, ctx.S, v.path_eval(), a);
}
template <class View>
void path_timing(const PlannerCtx &ctx, const View &v, const PathTimingArgs &a) {
  if (a.n_paths <= 0) return;
  use_device(ctx), path_timing_run(ctx.stream, ctx.S, v.path_eval(), a);
}
template <class View>
void body_query(const PlannerCtx &ctx, const View &v, const BodyArgs &a) {
  if (a.n_poses <= 0) return;
  use_device(ctx), body_query_run(ctx.stream, ctx.S, v.path_eval(), a);
}
template <class View>
void articulated_query(const PlannerCtx &ctx, const View &v, const ArticulatedArgs &a) {
  if (a.n_configs <= 0) return;
  use_device(ctx), articulated_query_run(ctx.stream, ctx.S, v.path_eval(), a);
}
template <class View>
void body_sweep(const PlannerCtx &ctx, const View &v, const SweepArgs &a) {
  if (a.n_paths <= 0) return;
  use_device(ctx), body_sweep_run(ctx.stream, ctx.S, v.path_eval(), a);
}

// The frontier call's store side: frontier_box gives the kernel's box, whether it is empty and (returned) the most entries it can yield,
// frontier_launch runs the store's kernel over a non-empty box.  Dense: the caller's box clipped to the array, local array coordinates
static int64_t frontier_box(const DenseView &v, const FrontierArgs &a, FrontierBox &b, bool &empty) {
  int64_t blo[3], bhi[3];
  empty = !v.clip_box(a.lo, a.hi, blo, bhi);
  b = FrontierBox{(int)blo[0], (int)blo[1], (int)blo[2], (int)bhi[0], (int)bhi[1], (int)bhi[2]};
  return empty ? 0 : (bhi[0] - blo[0] + 1) * (bhi[1] - blo[1] + 1) * (bhi[2] - blo[2] + 1);
}
static void frontier_launch(hipStream_t st, const DenseView &v, const FrontierBox &b, double min_clearance, const FrontierOut &out) {
  const int64_t nwords = (int64_t)(b.x1 - b.x0 + 1) * (b.y1 - b.y0 + 1) * ((b.z1 >> 5) - (b.z0 >> 5) + 1);
  hipLaunchKernelGGL(k_frontier_dense<DenseFrontierDist>, dim3(grid_for(nwords, 256, 8192)), dim3(256), 0, st, v.g, v.obs, v.occ, b, v.frontier(),
                     min_clearance, out);
}
// hash: every page; a null box is the whole map (pages lie within +-2^25: clamping to +-2^30 only keeps the kernel's differences in range)
static int64_t frontier_box(const HashView &v, const FrontierArgs &a, FrontierBox &b, bool &empty) {
  b = FrontierBox{clamp30(INT32_MIN), clamp30(INT32_MIN), clamp30(INT32_MIN), clamp30(INT32_MAX), clamp30(INT32_MAX), clamp30(INT32_MAX)};
  if (a.lo) b = FrontierBox{clamp30(a.lo[0]), clamp30(a.lo[1]), clamp30(a.lo[2]), clamp30(a.hi[0]), clamp30(a.hi[1]), clamp30(a.hi[2])};
  empty = b.x0 > b.x1 || b.y0 > b.y1 || b.z0 > b.z1 || v.npages == 0;
  return v.npages * kPageVox;
}
static void frontier_launch(hipStream_t st, const HashView &v, const FrontierBox &b, double min_clearance, const FrontierOut &out) {
  hipLaunchKernelGGL(k_frontier_hash<HashFrontierPages>, dim3(grid_for(v.npages, 1, 8192)), dim3(256), 0, st, v.page_gtile, v.npages, v.coc,
                     v.occbits, b, v.frontier(), min_clearance, out);
}
// dev: vox / mask / n_out_dev are device pointers and the call is only enqueued; else host pointers, and the total is returned
template <class View>
int64_t frontier_voxels(const PlannerCtx &ctx, const View &v, const FrontierArgs &a) {
  use_device(ctx);
  unsigned long long *count = a.dev ? a.n_out_dev : ctx.counter;
  hipLaunchKernelGGL(k_zero_words, dim3(1), dim3(64), 0, ctx.stream, count, 1);
  FIESTA_HIP_CHECK(hipGetLastError());
  FrontierBox b;
  bool empty;
  const int64_t cap = std::min(a.capacity, frontier_box(v, a, b, empty));
  Staging res{ctx.S.out, ctx.stream};  // (the host variant's)
  const auto vox = res.add(a.vox, 3 * cap);
  const auto mask = res.add(a.mask, cap);
  if (!a.dev) res.alloc();
  int32_t *dvox = a.dev ? a.vox : res.dev(vox);
  uint8_t *dmask = a.dev ? a.mask : res.dev(mask);
  if (!empty) {
    frontier_launch(ctx.stream, v, b, a.min_clearance, FrontierOut{dvox, dmask, (unsigned long long)cap, count});
    FIESTA_HIP_CHECK(hipGetLastError());
  }
  if (a.dev) return 0;
  FIESTA_HIP_CHECK(hipMemcpyAsync(ctx.counter_host, ctx.counter, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx.stream));
  FIESTA_HIP_CHECK(hipStreamSynchronize(ctx.stream));
  const int64_t n = (int64_t)*ctx.counter_host;
  res.back(vox, 3 * std::min(n, cap)), res.back(mask, std::min(n, cap));
  FIESTA_HIP_CHECK(hipStreamSynchronize(ctx.stream));
  return n;
}

// The skeleton call's store side, next to the frontier call's: the same box (frontier_box), the store's stencil kernel over it
static void skeleton_launch(hipStream_t st, const DenseView &v, const FrontierBox &b, const SkeletonArgs &a, const SkeletonOut &out) {
  const int64_t nrows = (int64_t)(b.x1 - b.x0 + 1) * (b.y1 - b.y0 + 1);  // a wave each, four to a work-group
  hipLaunchKernelGGL(k_skeleton_dense, dim3(grid_for(nrows, 4, 2048)), dim3(256), 0, st, v.g, v.field(), v.obs, v.occ, b,
                     a.min_sep2, a.min_clearance, out);
}
static void skeleton_launch(hipStream_t st, const HashView &v, const FrontierBox &b, const SkeletonArgs &a, const SkeletonOut &out) {
  hipLaunchKernelGGL(k_skeleton_hash<HashFrontierPages>, dim3(grid_for(v.npages, 1, 8192)), dim3(256), 0, st, v.page_gtile, v.npages, v.field(),
                     v.occbits, b, v.frontier(), a.min_sep2, a.min_clearance, out);
}
// dev: the result's arrays and n_out_dev are device pointers and the call is only enqueued; else host pointers, and the total is returned
template <class View>
int64_t skeleton_voxels(const PlannerCtx &ctx, const View &v, const SkeletonArgs &a) {
  use_device(ctx);
  unsigned long long *count = a.dev ? a.n_out_dev : ctx.counter;
  hipLaunchKernelGGL(k_zero_words, dim3(1), dim3(64), 0, ctx.stream, count, 1);
  FIESTA_HIP_CHECK(hipGetLastError());
  FrontierBox b;
  bool empty;
  const FrontierArgs box{a.lo, a.hi, a.min_clearance, nullptr, nullptr, a.capacity, nullptr, a.dev};
  const int64_t cap = std::min(a.capacity, frontier_box(v, box, b, empty));
  Staging res{ctx.S.out, ctx.stream};  // (the host variant's)
  const auto vox = res.add(a.res->vox, 3 * cap);
  const auto mask = res.add(a.res->mask, cap);
  const auto d2 = res.add(a.res->d2, cap);
  const auto sep2 = res.add(a.res->sep2, cap);
  if (!a.dev) res.alloc();
  const SkeletonOut out = a.dev ? SkeletonOut{a.res->vox, a.res->mask, a.res->d2, a.res->sep2, (unsigned long long)cap, count}
                                : SkeletonOut{res.dev(vox), res.dev(mask), res.dev(d2), res.dev(sep2), (unsigned long long)cap, count};
  if (!empty) {
    skeleton_launch(ctx.stream, v, b, a, out);
    FIESTA_HIP_CHECK(hipGetLastError());
  }
  if (a.dev) return 0;
  FIESTA_HIP_CHECK(hipMemcpyAsync(ctx.counter_host, ctx.counter, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx.stream));
  FIESTA_HIP_CHECK(hipStreamSynchronize(ctx.stream));
  const int64_t n = (int64_t)*ctx.counter_host, m = std::min(n, cap);
  res.back(vox, 3 * m), res.back(mask, m), res.back(d2, m), res.back(sep2, m);
  FIESTA_HIP_CHECK(hipStreamSynchronize(ctx.stream));
  return n;
}

template <class View>
void ray_query(const PlannerCtx &ctx, const View &v, const RayArgs &a) {
  if (a.n <= 0) return;
  use_device(ctx), ray_query_run(ctx.stream, ctx.S, v.ray_source(), a);
}
template <class View>
void reach_field(const PlannerCtx &ctx, const View &v, const ReachArgs &a) {
  use_device(ctx);
  int64_t blo[3], bhi[3];
  v.reach_box(a.lo, a.hi, blo, bhi);
  reach_run(ctx.stream, ctx.S, v.reach_source(), blo, bhi, v.off, a);
}
// reach_field's box and source
template <class View>
void reach_matrix(const PlannerCtx &ctx, const View &v, const ReachMatrixArgs &a) {
  use_device(ctx);
  int64_t blo[3], bhi[3];
  v.reach_box(a.lo, a.hi, blo, bhi);
  reach_matrix_run(ctx.stream, ctx.S, v.reach_source(), blo, bhi, v.off, a);
}
// reach_field's source over the store's window
template <class View>
void corridor(const PlannerCtx &ctx, const View &v, const CorridorArgs &a) {
  use_device(ctx);
  CorridorWin w{};
  v.corridor_window(a.lo, a.hi, w.lo, w.hi);
  for (int c = 0; c < 3; ++c) w.off[c] = v.off[c], w.org[c] = ctx.org[c];
  w.res = ctx.res;
  corridor_run(ctx.stream, ctx.S, v.reach_source(), w, a);
}
// the ray query's source, the frontier call's distance (in the coordinates the store's sources take)
template <class View>
void view_coverage(const PlannerCtx &ctx, const View &v, const ViewArgs &a) {
  use_device(ctx);
  const ViewSource<decltype(v.ray_source()), decltype(v.frontier())> vs{v.ray_source(), v.frontier(), {v.off[0], v.off[1], v.off[2]}};
  view_coverage_run(ctx.stream, ctx.S, vs, a);
}

#define FIESTA_PLANNER_CALLS(VIEW, MAP)                                                                                                   \
  template void path_clearance(const PlannerCtx &, const VIEW &, MAP::HostPathEval, const PathClearanceArgs &);                          \
  template void path_cost(const PlannerCtx &, const VIEW &, MAP::HostPathEval, const PathCostArgs &);                                    \
  template void path_refine(const PlannerCtx &, const VIEW &, const PathRefineArgs &);                                                   \
  template void path_timing(const PlannerCtx &, const VIEW &, const PathTimingArgs &);                                                   \
  template void body_query(const PlannerCtx &, const VIEW &, const BodyArgs &);                                                          \
  template void articulated_query(const PlannerCtx &, const VIEW &, const ArticulatedArgs &);                                            \
  template void body_sweep(const PlannerCtx &, const VIEW &, const SweepArgs &);                                                         \
  template int64_t frontier_voxels(const PlannerCtx &, const VIEW &, const FrontierArgs &);                                              \
  template int64_t skeleton_voxels(const PlannerCtx &, const VIEW &, const SkeletonArgs &);                                              \
  template void ray_query(const PlannerCtx &, const VIEW &, const RayArgs &);                                                            \
  template void reach_field(const PlannerCtx &, const VIEW &, const ReachArgs &);                                                        \
  template void reach_matrix(const PlannerCtx &, const VIEW &, const ReachMatrixArgs &);                                                 \
  template void corridor(const PlannerCtx &, const VIEW &, const CorridorArgs &);                                                        \
  template void view_coverage(const PlannerCtx &, const VIEW &, const ViewArgs &);
FIESTA_PLANNER_CALLS(DenseView, DenseMap)
FIESTA_PLANNER_CALLS(HashView, HashMap)
#undef FIESTA_PLANNER_CALLS

// ---- the calls that read no voxel -------------------------------------------------------------------------------------------------
void reach_paths(const PlannerCtx &ctx, const ReachPathArgs &a) { use_device(ctx), reach_paths_run(ctx.stream, ctx.S, ctx.res, ctx.org, a); }
void leg_paths(const PlannerCtx &ctx, const LegPathArgs &a) { use_device(ctx), leg_paths_run(ctx.stream, ctx.S, ctx.res, ctx.org, a); }
void cluster_voxels(const PlannerCtx &ctx, const ClusterArgs &a) { use_device(ctx), cluster_voxels_run(ctx.stream, ctx.S, ctx.res, ctx.org, a); }
void split_clusters(const PlannerCtx &ctx, const SplitArgs &a) { use_device(ctx), split_clusters_run(ctx.stream, ctx.S, ctx.res, ctx.org, a); }
void corridor_bounds(const PlannerCtx &ctx, const CorridorBoundsArgs &a) {
  if (a.n_paths <= 0) return;
  use_device(ctx), corridor_bounds_run(ctx.stream, ctx.S, a);
}
void site_tour(const PlannerCtx &ctx, const TourArgs &a) { use_device(ctx), site_tour_run(ctx.stream, ctx.S, a); }

}  // namespace fiesta
