// fiesta_amd/csrc/planner.hpp -- what a map keeps for the planner calls, and the calls themselves.
//
// Both stores own one PlannerScratch.  The twenty calls are the free functions at the end of this header, defined once in
// planner.hip, the only unit that includes the planner kernel headers: six need nothing of a map but its planner_ctx(); fourteen also
// read voxels, through the store's planner_view() (dense_read.hpp: DenseView, hash_read.hpp: HashView).
#pragma once
#include <algorithm>

#include "../../include/fiesta_hip.h"
#include "common.hpp"

namespace fiesta {

// the reach calls' limit on the voxels of their clipped box: keeps every cost below 2^31 (5 * 2^28) and bounds the scratch
constexpr int64_t kReachMaxVoxels = 1ll << 28;

// scratch of fiesta_hip_reach_field (reach_kernels.hpp), owned by a map: the box's traversability bitmap, tile flags and lists of
// both round parities, the counters, and a cost field for calls that pass none; allocated on first use, freed with the map.
// field_*: what `cost` holds for fiesta_hip_reach_paths (reach_path_kernels.hpp) -- the RETAINED field: valid after a reach_field
// call that finished with its cost field in this scratch, or after a reach_paths host call uploaded one; its inclusive box in map
// voxel coordinates and the connectivity it was flooded with
struct ReachScratch {
  DevBuf<uint32_t> bits, flags, lists;
  DevBuf<int32_t> cost;
  DevBuf<unsigned long long> ctr;
  bool field_valid = false;
  int32_t field_lo[3] = {0, 0, 0}, field_hi[3] = {0, 0, 0};
  int field_connectivity = 0;
};

// scratch of fiesta_hip_reach_matrix (reach_matrix_kernels.hpp), owned by a map: the cost planes of one batch of floods, the flags and
// lists of their (flood, tile) items for both round parities, the counters, and the per-source status and reached counts; allocated
// on first use, grown on demand, freed with the map.  (The bitmap is ReachScratch::bits; ReachScratch::cost is never touched.)
// batch_*: what `planes` holds for fiesta_hip_leg_paths (leg_path_kernels.hpp) -- the RETAINED batch: valid after a reach_matrix call
// that succeeded with at least one source, a non-empty box and all sources in ONE batch (plane s is source s's flood, `status` its
// per-source status); its inclusive box in map voxel coordinates, its connectivity, the number of sources and `sites`, the
// call's own copy of the source voxels.  batch_why says what the last call left when it left no batch.
struct ReachMatrixScratch {
  enum { kNoCallYet = 0, kManyBatches = 1, kNothingToKeep = 2 };
  DevBuf<int32_t> planes, status, sites;
  DevBuf<uint32_t> flags, lists;
  DevBuf<unsigned long long> ctr, reached;
  bool batch_valid = false;
  int batch_why = kNoCallYet;
  int32_t batch_lo[3] = {0, 0, 0}, batch_hi[3] = {0, 0, 0};
  int batch_connectivity = 0;
  int64_t batch_sources = 0;
};

// scratch of fiesta_hip_site_tour (tour_kernels.hpp), owned by a map: the call's header words and info, the visited sites and the
// statuses, the compact m x m matrix, and per restart its final tour, length, moves and capped flag; allocated on first use, grown
// on demand, freed with the map; no other call touches it
struct TourScratch {
  DevBuf<int32_t> head, site, status, mat, tours, stat;
  DevBuf<long long> len;
};

// scratch of fiesta_hip_cluster_voxels (cluster_kernels.hpp), owned by a map: the voxel hash table, the per-entry union-find arrays,
// the per-cluster accumulators and two counters; allocated on first use, grown on demand, freed with the map
struct ClusterScratch {
  DevBuf<unsigned long long> keys, sum, kmin, ctr;
  DevBuf<int32_t> tidx, lab, parent, cnt, box, csize;
  DevBuf<uint32_t> mor;
};

// scratch of fiesta_hip_split_clusters (split_kernels.hpp), owned by a map, O(n_members): three pools that one call carves into the two
// member / part buffer sets, the per-part records, boxes and accumulators, the flag bytes, their scan and the counters
struct SplitScratch {
  DevBuf<int32_t> i32;
  DevBuf<unsigned long long> u64;
  DevBuf<uint8_t> u8;
};

// scratch of fiesta_hip_view_coverage (view_kernels.hpp), owned by a map: the ring form's expanded views, the per-view pair counts
// and their scan, the per-view and per-group accumulators and four counters; O(views + groups), grown on demand, freed with the map
struct ViewScratch {
  DevBuf<int64_t> P;
  DevBuf<int32_t> vin, vvis, group;
  DevBuf<unsigned long long> best, ctr;
  DevBuf<double> pos, dir;
  DevBuf<unsigned char> call;  // one ViewCall
};

// what a map keeps between calls for them, one per map: the staged inputs of a host variant (every host-pointer call of the ABI
// stages here), the path calls' plan / piece records, the staged outputs, and the four planner calls' own scratch
struct PlannerScratch {
  DevBuf<unsigned char> in, tmp, out;
  ReachScratch reach;
  ReachMatrixScratch reach_matrix;
  TourScratch tour;
  ClusterScratch cluster;
  SplitScratch split;
  ViewScratch view;
};

// A host variant's staged sections in one of PlannerScratch's buffers (in: what goes up, out: what comes back): add() every
// section (8-byte aligned, in order), alloc(), then dev() / up() / back().  A section whose host pointer is null has no device
// pointer and is never copied.  Every call synchronises before it returns, so the next call finds both buffers free.
struct Staging {
  template <typename T>
  struct Sec {
    T *host;
    size_t off;
  };
  DevBuf<unsigned char> &buf;
  hipStream_t st;
  size_t end = 0;
  static size_t up8(size_t b) { return (b + 7) / 8 * 8; }
  template <typename T>
  Sec<T> add(T *host, size_t count) {
    const Sec<T> s{host, end};
    end += up8(count * sizeof(T));
    return s;
  }
  void alloc(size_t keep = 0) { buf.ensure(std::max<size_t>(end, 8), st, keep); }  // keep: bytes of an earlier alloc() to preserve
  template <typename T>
  T *dev(const Sec<T> &s) const {
    return s.host ? (T *)(buf.p + s.off) : nullptr;
  }
  template <typename T>
  void up(const Sec<T> &s, size_t count) const {
    if (s.host && count) FIESTA_HIP_CHECK(hipMemcpyAsync(buf.p + s.off, s.host, count * sizeof(T), hipMemcpyHostToDevice, st));
  }
  template <typename T>
  void back(const Sec<T> &s, size_t count) const {
    if (s.host && count) FIESTA_HIP_CHECK(hipMemcpyAsync(s.host, buf.p + s.off, count * sizeof(T), hipMemcpyDeviceToHost, st));
  }
};

// the planner calls' arguments as the C ABI takes them, already checked: defined in planner_args.hpp, built once by c_api.hip.
// (Named only: raycast.hip sees the stores' headers and keeps a RayArgs of its own.)
template <typename R>
struct PathArgs;
struct BodyArgs;
struct ArticulatedArgs;
struct SweepArgs;
struct FrontierArgs;
struct SkeletonArgs;
struct RayArgs;
struct ReachArgs;
struct ReachMatrixArgs;
struct ReachPathArgs;
struct LegPathArgs;
struct CorridorArgs;
struct PathRefineArgs;
struct PathTimingArgs;
struct CorridorBoundsArgs;
struct TourArgs;
struct ClusterArgs;
struct SplitArgs;
struct ViewArgs;

// ---- the planner calls (planner.hip) ------------------------------------------------------------------------------------------------
// what every call takes of a map, either store's planner_ctx(): its device and stream, its scratch, its resolution and origin, and
// a counter of the map's (the C_SCRATCH slot) with its pinned host mirror, for a host variant's total
struct PlannerCtx {
  int device;
  hipStream_t stream;
  PlannerScratch &S;
  double res;
  const double *org;
  unsigned long long *counter, *counter_host;
};
// The calls that read voxels.  View: DenseView (dense_read.hpp) or HashView (hash_read.hpp), the store's planner_view(), which prepares
// what the kernels read; planner.hip instantiates each call for both.  fiesta_hip_path_clearance[_dev] and fiesta_hip_path_cost[_dev] (host:
// the store's host_path_eval(), which answers a small host batch from its brick cache), fiesta_hip_path_refine[_dev], fiesta_hip_path_timing[_dev]
template <class View, class HostEval>
void path_clearance(const PlannerCtx &ctx, const View &v, HostEval host, const PathArgs<fiesta_hip_path_result> &a);
template <class View, class HostEval>
void path_cost(const PlannerCtx &ctx, const View &v, HostEval host, const PathArgs<fiesta_hip_path_cost_result> &a);
template <class View>
void path_refine(const PlannerCtx &ctx, const View &v, const PathRefineArgs &a);
template <class View>
void path_timing(const PlannerCtx &ctx, const View &v, const PathTimingArgs &a);
// fiesta_hip_body_query[_dev]: the path calls' evaluator at the sphere centres of a body (always on the device)
template <class View>
void body_query(const PlannerCtx &ctx, const View &v, const BodyArgs &a);
// fiesta_hip_articulated_query[_dev]: the same at the spheres of several frames, one pose per frame (always on the device)
template <class View>
void articulated_query(const PlannerCtx &ctx, const View &v, const ArticulatedArgs &a);
// fiesta_hip_body_sweep[_dev]: the same along CSR polylines of poses, sampled and reduced per path (always on the device)
template <class View>
void body_sweep(const PlannerCtx &ctx, const View &v, const SweepArgs &a);
// fiesta_hip_get_frontier_voxels[_dev]: returns the host variant's total (which may exceed the capacity)
template <class View>
int64_t frontier_voxels(const PlannerCtx &ctx, const View &v, const FrontierArgs &a);
// fiesta_hip_get_skeleton_voxels[_dev]: returns the host variant's total (which may exceed the capacity)
template <class View>
int64_t skeleton_voxels(const PlannerCtx &ctx, const View &v, const SkeletonArgs &a);
// fiesta_hip_ray_query[_dev], fiesta_hip_reach_field[_dev], fiesta_hip_reach_matrix[_dev], fiesta_hip_free_boxes[_dev] and
// fiesta_hip_path_corridor[_dev], fiesta_hip_view_coverage[_dev]
template <class View>
void ray_query(const PlannerCtx &ctx, const View &v, const RayArgs &a);
template <class View>
void reach_field(const PlannerCtx &ctx, const View &v, const ReachArgs &a);
template <class View>
void reach_matrix(const PlannerCtx &ctx, const View &v, const ReachMatrixArgs &a);
template <class View>
void corridor(const PlannerCtx &ctx, const View &v, const CorridorArgs &a);
template <class View>
void view_coverage(const PlannerCtx &ctx, const View &v, const ViewArgs &a);
// The calls that read no voxel.  fiesta_hip_reach_paths[_dev], fiesta_hip_leg_paths[_dev] (the batch the last reach_matrix call
// retained), fiesta_hip_cluster_voxels[_dev] and fiesta_hip_split_clusters[_dev]: nothing of the map is read but its resolution and origin
void reach_paths(const PlannerCtx &ctx, const ReachPathArgs &a);
void leg_paths(const PlannerCtx &ctx, const LegPathArgs &a);
void cluster_voxels(const PlannerCtx &ctx, const ClusterArgs &a);
void split_clusters(const PlannerCtx &ctx, const SplitArgs &a);
// fiesta_hip_corridor_bounds[_dev] and fiesta_hip_site_tour[_dev]: nothing of the map is read at all
void corridor_bounds(const PlannerCtx &ctx, const CorridorBoundsArgs &a);
void site_tour(const PlannerCtx &ctx, const TourArgs &a);

}  // namespace fiesta

