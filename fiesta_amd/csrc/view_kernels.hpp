// fiesta_amd/csrc/view_kernels.hpp -- view coverage: fiesta_hip_view_coverage / _dev (include/fiesta_hip.h).
//
// The step after the cluster call: candidate viewpoints (explicit, or a ring of offsets around every cluster centroid) against the
// member voxels of their cluster -- per (view, member) pair the sensor's range and field-of-view test, then the ray query's walk
// from the view to the member's centre, ended by the first blocking voxel; counted per view, per target and per group.  Passes, all
// on the map's stream, none cooperative, no work-group ever waits for another:
//   k_view_setup     the call's arguments into device memory (see ViewCall)
//   k_view_init      per-target and per-group identities, the four counters
//   k_view_ring      ring form only: explicit views (pos, dir, group) into the scratch; one code path from here on
//   k_view_pass<S>   per view: usable? (finite, group in range, voxel FREE, clearance), its class, its pair count P[v] (the group's
//                    size if usable, else 0), its two counters at 0 (usable) or -1
//   k_view_scan      ONE work-group striding with a carry (the shape of k_cluster_number): exclusive int64 scan of P, V + 1 entries
//   k_view_pairs<S>  the hot path.  The flat pair index space [0, P[V]) in batches of kViewBatch tiles of 256, dealt to work-groups
//                    grid-stride; the total is read on the device.  Per tile a lane finds its view (the wave's first view is the
//                    previous tile's unless the tile starts past its end, then one uniform bisection of P from there; a lane's own
//                    view by a second bisection only if it lies beyond; the first view's range and segment sit in scalar
//                    registers), forms q and runs the range / field-of-view cull.  Survivors are appended to an LDS queue of
//                    (view, entry): wave ballot, prefix popcount, one LDS atomicAdd per wave.  The queue is CARRIED across a
//                    work-group's batches: after a batch it is walked 256 pairs at a time only while it holds that many, the rest
//                    waits for the next batch, and everything left goes after the last one.  So the divergent dda_walk runs on full
//                    waves where a work-group has batches enough to fill the queue (a call of more than 2048 batches; with a
//                    survival rate s a drain needs 256 / (1024 s) batches), and on one partial drain per work-group otherwise.
//                    Per-view counts: per wave over the DISTINCT views present (wave_count_keys of wave_ops.hpp),
//                    one atomicAdd per wave, view and quantity.  cover_count: atomicAdd; first_view: unsigned atomicMin (-1 is
//                    the identity).  The totals: one atomicAdd per wave.
//   k_view_finish    per view: the counts out; one packed 64-bit atomicMax (n_visible << 32 | ~index) into its group
//   k_view_groups    per group: unpack; the totals into info
// Every reduction is an integer sum, minimum or maximum: the outputs are the same bits for any launch shape and scheduling, and the
// bits of fiesta_amd.view_coverage_model.  LDS: the queue (10 KiB) and the scan's wave totals.  No scratch memory.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>

#include "../../include/fiesta_hip.h"
#include "common.hpp"
#include "planner.hpp"
#include "planner_args.hpp"
#include "ray_query_kernels.hpp"
#include "ray_walk.hpp"
#include "wave_ops.hpp"

namespace fiesta {
namespace {  // (planner.hip alone includes this header; the namespace is part of the kernels' symbol names)

constexpr int kViewBlock = 256, kViewMaxBlocks = 2048;
constexpr int kViewBatch = 4;                         // tiles per batch
constexpr int kViewQueueBatch = kViewBlock * kViewBatch;      // pairs per batch
constexpr int kViewQueue = kViewQueueBatch + kViewBlock;      // the LDS queue: up to 255 pairs left over and every pair of a batch
constexpr int kViewScanBlock = 1024, kViewScanItems = 4;

// what the view pass needs of a map beside the ray source: GetDistance(Vector3i) for the clearance rule.  DIST takes the
// coordinates the frontier kernel hands it: map voxel minus d0 (dense maps: local array coordinates; hash-block maps: d0 = 0)
template <class SRC, class DIST>
struct ViewSource {
  using Ray = SRC;
  SRC ray;
  DIST dist;
  int d0[3];
};

struct ViewIn {  // device pointers
  const int32_t *vox;
  const int64_t *offsets, *members;  // nullable
  const int64_t *n_groups_dev;       // nullable
  int64_t n, n_groups, n_members;    // n_groups: 1 if offsets is null; n_members: n if members is null
  const double *pos, *dir;           // V x 3, V x 2 (dir nullable with OMNI)
  const int32_t *group;              // V, nullable
  int64_t V;
};
struct ViewSensor {
  double min2, max2, tan_h, tan_v, min_clearance;
  int block_mask, omni, min_visible;
};
struct ViewWork {  // device view of the map's ViewScratch for one call
  int64_t *P;                // V + 1: pair counts, then their exclusive scan
  int32_t *vin, *vvis;       // V: pairs in view / visible; -1: unusable view
  unsigned long long *best;  // n_groups
  unsigned long long *ctr;   // [0] usable views, [1] pairs, [2] in view, [3] visible
};

// One call's arguments in device memory (ViewScratch::call).  The view pass and the pair kernel read them through a pointer: as kernel
// arguments they would sit in some sixty scalar registers from entry to exit, next to the ray source the walk needs, and the
// register allocator would spill; read where they are used, each phase holds only its own.
struct ViewCall {
  ViewWork w;
  ViewIn in;
  ViewSensor sn;
  fiesta_hip_view_result o;
};
__global__ void k_view_setup(ViewCall *dst, ViewCall c) {
  if (threadIdx.x == 0) *dst = c;
}

__device__ inline int64_t view_groups(const ViewIn &in) {
  if (!in.n_groups_dev) return in.n_groups;
  const int64_t d = *in.n_groups_dev;
  return d < in.n_groups ? (d < 0 ? 0 : d) : in.n_groups;
}
__device__ inline int64_t view_clamp(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
// the member segment of group g: [lo, lo + size)
__device__ inline int64_t view_segment(const ViewIn &in, int64_t g, int64_t &lo) {
  lo = 0;
  if (!in.offsets) return in.n_members;
  lo = view_clamp(in.offsets[g], in.n_members);
  const int64_t hi = view_clamp(in.offsets[g + 1], in.n_members);
  return hi > lo ? hi - lo : 0;
}

__global__ __launch_bounds__(kViewBlock) void k_view_init(ViewWork w, ViewIn in, fiesta_hip_view_result o) {
  const int64_t stride = (int64_t)gridDim.x * kViewBlock, t = blockIdx.x * (int64_t)kViewBlock + threadIdx.x;
  for (int64_t i = t; i < in.n; i += stride) {
    if (o.cover_count) o.cover_count[i] = 0;
    if (o.first_view) o.first_view[i] = -1;
  }
  for (int64_t g = t; g < in.n_groups; g += stride) w.best[g] = 0;
  if (t < 4) w.ctr[t] = 0;
}

__global__ __launch_bounds__(kViewBlock) void k_view_ring(const double *centroid, const double *ring, int64_t n_groups, int64_t n_ring, double *pos,
                                                          double *dir, int32_t *group) {
  const int64_t V = n_groups * n_ring, stride = (int64_t)gridDim.x * kViewBlock;
  for (int64_t v = blockIdx.x * (int64_t)kViewBlock + threadIdx.x; v < V; v += stride) {
    const int64_t k = v / n_ring, j = v % n_ring;
#pragma unroll
    for (int c = 0; c < 3; ++c) pos[3 * v + c] = centroid[3 * k + c] + ring[5 * j + c];
    dir[2 * v] = ring[5 * j + 3], dir[2 * v + 1] = ring[5 * j + 4];
    group[v] = (int32_t)k;
  }
}

// the class of walk voxel (x, y, z): the map voxel v of its centre in the ray query's arithmetic (k_ray_query's visit), then SRC
template <class SRC>
__device__ inline int view_classify(const SRC &src, typename SRC::Cache &cache, int x, int y, int z, int *v) {
  const double res = src.g.res;
  const double p[3] = {(x + 0.5) * res, (y + 0.5) * res, (z + 0.5) * res};
  for (int c = 0; c < 3; ++c)  // Pos2Vox, saturated
    v[c] = (int)fmin(fmax(floor((p[c] - src.g.org[c]) / res), -2147483647.0), 2147483647.0);
  const int rr[3] = {x, y, z};
  return src.classify(rr, v, cache);
}

template <class VS>
__global__ __launch_bounds__(kViewBlock) void k_view_pass(VS s, const ViewCall *call) {
  const ViewWork &w = call->w;
  const ViewIn &in = call->in;
  const ViewSensor &sn = call->sn;
  const fiesta_hip_view_result &o = call->o;
  const int64_t G = view_groups(in), stride = (int64_t)gridDim.x * kViewBlock;
  const double res = s.ray.g.res;
  for (int64_t base = blockIdx.x * (int64_t)kViewBlock + (threadIdx.x & ~63); base < in.V; base += stride) {  // (whole waves: the ballot)
    const int64_t v = base + (threadIdx.x & 63);
    bool usable = false;
    if (v < in.V) {
      double a[3];
      bool ok = true;
      for (int c = 0; c < 3; ++c) {
        const double pc = in.pos[3 * v + c];
        a[c] = pc / res;
        ok = ok && fabs(pc) < (double)INFINITY && fabs(a[c]) < kRayMaxCoord;  // (a NaN fails the comparison as well)
      }
      int cls = 0;
      int64_t size = 0;
      if (ok) {
        int mv[3];
        typename VS::Ray::Cache cache = VS::Ray::fresh();
        cls = view_classify(s.ray, cache, (int)floor(a[0]), (int)floor(a[1]), (int)floor(a[2]), mv);
        const int64_t g = in.group ? (int64_t)in.group[v] : 0;
        usable = cls == FIESTA_HIP_RAY_FREE && g >= 0 && g < G;
        if (usable && sn.min_clearance > 0) usable = s.dist(mv[0] - s.d0[0], mv[1] - s.d0[1], mv[2] - s.d0[2]) >= sn.min_clearance;
        if (usable) {
          int64_t lo;
          size = view_segment(in, g, lo);
        }
      }
      if (o.view_class) o.view_class[v] = (uint8_t)cls;
      w.P[v] = size;
      w.vin[v] = w.vvis[v] = usable ? 0 : -1;
    }
    const unsigned long long b = __ballot(usable);
    if (b && (threadIdx.x & 63) == 0) atomicAdd(&w.ctr[0], (unsigned long long)__popcll(b));
  }
}

// exclusive scan of P[0 .. V] in place (P[V] is written with the total); one work-group, the carry in a register
__global__ __launch_bounds__(kViewScanBlock) void k_view_scan(ViewWork w, int64_t V) {
  __shared__ long long s_wave[kViewScanBlock / 64];
  const long long total = block_scan_stride<kViewScanItems, kViewScanBlock / 64>(
      V, s_wave, [&](int64_t v) { return (long long)w.P[v]; }, [&](int64_t v, long long before, long long) { w.P[v] = before; });
  if (threadIdx.x == 0) w.P[V] = total, w.ctr[1] = (unsigned long long)total;
}

// the view of pair index idx: the largest v with P[v] <= idx (views without pairs share their successor's P and are skipped)
__device__ inline int view_find(const int64_t *P, int64_t V, int64_t idx, int64_t lo) {
  int64_t hi = V;  // P[lo] <= idx < P[hi]
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (P[mid] <= idx)
      lo = mid;
    else
      hi = mid;
  }
  return (int)lo;
}

template <class SRC>
__global__ __launch_bounds__(kViewBlock) void k_view_pairs(SRC src, const ViewCall *call) {
  const ViewWork &w = call->w;
  const ViewIn &in = call->in;
  const ViewSensor &sn = call->sn;
  const fiesta_hip_view_result &o = call->o;
  __shared__ int s_qview[kViewQueue], s_qent[kViewQueue];
  __shared__ int s_qn;
  const int tid = threadIdx.x, lane = tid & 63;
  const double res = src.g.res;
  const int64_t total = w.P[in.V], nbatches = (total + kViewQueueBatch - 1) / kViewQueueBatch;
  const int64_t groups = gridDim.x;
  if (blockIdx.x >= nbatches) return;  // (uniform per work-group, before any barrier)
  int vprev = 0;                       // the wave's first view of its previous tile: pair indices only grow, so the search starts there
  if (tid == 0) s_qn = 0;
  __syncthreads();
  for (int64_t batch = blockIdx.x;; batch += groups) {  // (uniform per work-group)
    const bool more = batch < nbatches;
    // ---- the cull: kViewBatch tiles of 256 pairs, survivors appended to the queue (below 256 entries are left from earlier batches)
    for (int t = 0; more && t < kViewBatch; ++t) {
      const int64_t wave0 = (batch * kViewBatch + t) * kViewBlock + (tid & ~63);  // the wave's first pair
      if (wave0 >= total) break;                                                  // (uniform per wave; no barrier inside this loop)
      const int64_t idx = wave0 + lane;
      bool keep = false;
      int view = 0, ent = 0;
      // the wave's first view, its range of pairs and its segment: the same for every lane, held in scalar registers
      int v0 = vprev;                  // P[vprev] <= wave0; inside a large group the next test is the whole search
      if (wave0 >= w.P[v0 + 1]) v0 = view_find(w.P, in.V, wave0, v0);
      v0 = vprev = __builtin_amdgcn_readfirstlane(v0);
      const int64_t p1 = w.P[v0 + 1];  // (P[V] = total > wave0: v0 + 1 <= V)
      int64_t first = w.P[v0], lo;
      (void)view_segment(in, in.group ? (int64_t)in.group[v0] : 0, lo);
      if (idx < total) {
        view = v0;
        if (idx >= p1) {  // this lane lies in a later view
          view = view_find(w.P, in.V, idx, v0);
          first = w.P[view];
          (void)view_segment(in, in.group ? (int64_t)in.group[view] : 0, lo);
        }
        const int64_t m = lo + (idx - first);  // < n_members: P[view + 1] - P[view] is the clamped size
        const int64_t e = in.members ? in.members[m] : m;
        if (e >= 0 && e < in.n) {
          ent = (int)e;
          double q[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) q[c] = (((double)in.vox[3 * e + c] + 0.5) * res + src.g.org[c]) - in.pos[3 * (int64_t)view + c];
          const double d2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2];
          if (sn.min2 <= d2 && d2 <= sn.max2) {
            if (sn.omni) {
              keep = fabs(q[2]) <= sn.tan_v * sqrt(q[0] * q[0] + q[1] * q[1]);
            } else {
              const double dx = in.dir[2 * (int64_t)view], dy = in.dir[2 * (int64_t)view + 1];
              const double fwd = q[0] * dx + q[1] * dy, lat = q[1] * dx - q[0] * dy;
              keep = fwd > 0 && fabs(lat) <= sn.tan_h * fwd && fabs(q[2]) <= sn.tan_v * fwd;
            }
          }
        }
      }
      const unsigned long long b = __ballot(keep);
      if (b) {  // (uniform per wave)
        int at = 0;
        if (lane == 0) at = atomicAdd(&s_qn, __popcll(b)), atomicAdd(&w.ctr[2], (unsigned long long)__popcll(b));
        at = __shfl(at, 0) + __popcll(b & ((1ull << lane) - 1));
        if (keep) s_qview[at] = view, s_qent[at] = ent;  // at < kViewQueue: at most 255 left over + the kViewQueueBatch pairs of a batch
        wave_count_keys(w.vin, keep, view);
      }
    }
    __syncthreads();
    // ---- the walks: 256 queued pairs at a time while there are that many; what is left waits for the next batch, and after the
    //      last batch everything goes
    int qn = s_qn;
    __syncthreads();  // (everyone holds the count before a wave that runs ahead appends the next batch's pairs)
    const int at_least = more ? kViewBlock : 1;
    bool drained = false;
    while (qn >= at_least) {  // (uniform per work-group)
      const int take = min(qn, kViewBlock);
      qn -= take;
      drained = true;
      bool vis = false;
      int view = 0, ent = 0;
      if (tid < take) {
        view = s_qview[qn + tid], ent = s_qent[qn + tid];
        double a[3], b[3];
        bool ok = true;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double p = ((double)in.vox[3 * (int64_t)ent + c] + 0.5) * res + src.g.org[c];
          a[c] = in.pos[3 * (int64_t)view + c] / res;  // (finite and below 2^30: the view is usable)
          b[c] = p / res;
          ok = ok && fabs(p) < (double)INFINITY && fabs(b[c]) < kRayMaxCoord;
        }
        if (ok) {
          const int64_t m = llabs((int64_t)floor(b[0]) - (int64_t)floor(a[0])) + llabs((int64_t)floor(b[1]) - (int64_t)floor(a[1])) +
                            llabs((int64_t)floor(b[2]) - (int64_t)floor(a[2]));
          ok = m <= kRayMaxManhattan;
        }
        if (ok) {
          typename SRC::Cache cache = SRC::fresh();
          bool blocked = false;
          auto visit = [&](int x, int y, int z, int, bool last) -> bool {
            if (last) return true;  // the target's own voxel: never tested
            int mv[3];
            blocked = (view_classify(src, cache, x, y, z, mv) & sn.block_mask) != 0;
            return blocked;
          };
          (void)dda_walk<false, false>(a, b, nullptr, nullptr, visit);  // (0: both ends in one voxel, nothing to test)
          vis = !blocked;
        }
      }
      const unsigned long long b = __ballot(vis);
      if (b) {  // (uniform per wave)
        if (lane == 0) atomicAdd(&w.ctr[3], (unsigned long long)__popcll(b));
        wave_count_keys(w.vvis, vis, view);
        if (vis && o.cover_count) atomicAdd(&o.cover_count[ent], 1);
        if (vis && o.first_view) atomicMin((unsigned int *)&o.first_view[ent], (unsigned int)view);
      }
    }
    if (!more) break;
    if (drained) {  // (uniform per work-group) the entries taken are read: the next batch appends behind what is left
      __syncthreads();
      if (tid == 0) s_qn = qn;
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(kViewBlock) void k_view_finish(ViewWork w, ViewIn in, ViewSensor sn, fiesta_hip_view_result o) {
  const int64_t stride = (int64_t)gridDim.x * kViewBlock;
  for (int64_t v = blockIdx.x * (int64_t)kViewBlock + threadIdx.x; v < in.V; v += stride) {
    const int nin = w.vin[v], nvis = w.vvis[v];
    if (o.n_in_view) o.n_in_view[v] = nin;
    if (o.n_visible) o.n_visible[v] = nvis;
    if (nvis >= sn.min_visible)  // (usable, so its group is below the effective count <= n_groups)
      atomicMax(&w.best[in.group ? in.group[v] : 0], ((unsigned long long)(uint32_t)nvis << 32) | (unsigned long long)(~(uint32_t)v));
  }
}

__global__ __launch_bounds__(kViewBlock) void k_view_groups(ViewWork w, ViewIn in, fiesta_hip_view_result o, fiesta_hip_view_info *info) {
  const int64_t stride = (int64_t)gridDim.x * kViewBlock, t = blockIdx.x * (int64_t)kViewBlock + threadIdx.x;
  for (int64_t g = t; g < in.n_groups; g += stride) {
    const unsigned long long b = w.best[g];
    if (o.best_view) o.best_view[g] = b ? (int64_t)(~(uint32_t)(b & 0xFFFFFFFFull)) : -1;
    if (o.best_count) o.best_count[g] = (int32_t)(b >> 32);
  }
  if (t == 0 && info)
    info->n_usable = (int64_t)w.ctr[0], info->n_pairs = (int64_t)w.ctr[1], info->n_in_view = (int64_t)w.ctr[2], info->n_visible = (int64_t)w.ctr[3];
}

inline int64_t view_count_of(const ViewArgs &a) { return a.views->pos ? a.views->n_views : (a.offsets ? a.n_groups : 1) * a.views->n_ring; }

// enqueue the passes; every pointer of `in` (but centroid / ring: device pointers too), `o` and info is a device pointer
template <class VS>
void view_enqueue(hipStream_t st, ViewScratch &S, const VS &vs, ViewIn in, const double *centroid, const double *ring, int64_t n_ring,
                  const fiesta_hip_view_sensor &sensor, const fiesta_hip_view_result &o, fiesta_hip_view_info *info) {
  const int64_t V = in.V, G = in.n_groups;
  S.P.ensure((size_t)V + 1, st), S.vin.ensure((size_t)std::max<int64_t>(V, 1), st), S.vvis.ensure((size_t)std::max<int64_t>(V, 1), st);
  S.best.ensure((size_t)std::max<int64_t>(G, 1), st), S.ctr.ensure(4, st);
  if (!in.pos) {
    S.pos.ensure((size_t)std::max<int64_t>(3 * V, 1), st), S.dir.ensure((size_t)std::max<int64_t>(2 * V, 1), st), S.group.ensure((size_t)std::max<int64_t>(V, 1), st);
    in.pos = S.pos.p, in.dir = S.dir.p, in.group = S.group.p;
  }
  S.call.ensure(sizeof(ViewCall), st);
  const ViewWork w{S.P.p, S.vin.p, S.vvis.p, S.best.p, S.ctr.p};
  const ViewSensor sn{sensor.min_range * sensor.min_range, sensor.max_range * sensor.max_range, sensor.tan_h, sensor.tan_v, sensor.min_clearance,
                      sensor.block_mask, (sensor.flags & FIESTA_HIP_VIEW_OMNI) ? 1 : 0, sensor.min_visible};
  const auto blocks = [](int64_t items) { return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((items + kViewBlock - 1) / kViewBlock, kViewMaxBlocks))); };
  const ViewCall *call = (const ViewCall *)S.call.p;
  hipLaunchKernelGGL(k_view_setup, dim3(1), dim3(64), 0, st, (ViewCall *)S.call.p, ViewCall{w, in, sn, o});
  hipLaunchKernelGGL(k_view_init, blocks(std::max(in.n, G)), dim3(kViewBlock), 0, st, w, in, o);
  if (V > 0) {
    if (centroid) hipLaunchKernelGGL(k_view_ring, blocks(V), dim3(kViewBlock), 0, st, centroid, ring, G, n_ring, S.pos.p, S.dir.p, S.group.p);
    hipLaunchKernelGGL(k_view_pass<VS>, blocks(V), dim3(kViewBlock), 0, st, vs, call);
  }
  hipLaunchKernelGGL(k_view_scan, dim3(1), dim3(kViewScanBlock), 0, st, w, V);
  if (V > 0 && in.n > 0 && in.n_members > 0) {
    // (an upper bound of the pair count sizes the grid: the count itself stays on the device)
    const int64_t per = kViewBlock * kViewBatch, most = V * in.n_members;
    const int64_t nb = std::max<int64_t>(1, std::min<int64_t>((most + per - 1) / per, kViewMaxBlocks));
    hipLaunchKernelGGL(k_view_pairs<typename VS::Ray>, dim3((unsigned)nb), dim3(kViewBlock), 0, st, vs.ray, call);
  }
  if (V > 0) hipLaunchKernelGGL(k_view_finish, blocks(V), dim3(kViewBlock), 0, st, w, in, sn, o);
  hipLaunchKernelGGL(k_view_groups, blocks(G), dim3(kViewBlock), 0, st, w, in, o, info);
  FIESTA_HIP_CHECK(hipGetLastError());
}

// Both variants of the call on a map's stream.  The device variant only enqueues.  The host variant stages the inputs through
// P.in and every output through P.out, synchronises and copies back.
template <class VS>
void view_coverage_run(hipStream_t st, PlannerScratch &P, const VS &vs, const ViewArgs &a) {
  ViewScratch &S = P.view;
  const fiesta_hip_view_result none{};
  const fiesta_hip_view_result &r = a.res ? *a.res : none;
  const fiesta_hip_view_set &vw = *a.views;
  const int64_t G = a.offsets ? a.n_groups : 1, V = view_count_of(a), NM = a.members ? a.n_members : a.n;
  if (a.dev) {
    const ViewIn vi{a.vox, a.offsets, a.members, a.n_groups_dev, a.n, G, NM, vw.pos, vw.dir, vw.group, V};
    view_enqueue(st, S, vs, vi, vw.pos ? nullptr : vw.centroid, vw.ring, vw.n_ring, *a.sensor, r, a.info);
    return;
  }
  const size_t n = (size_t)a.n, g = (size_t)G, v = (size_t)V, nm = (size_t)NM, ring = vw.pos ? 0 : (size_t)vw.n_ring;
  Staging in{P.in, st}, out{P.out, st};
  // exactly one of pos and centroid is given; dir and group belong to the explicit form, and the other form's ring is empty
  const auto offsets = in.add(a.offsets, g + 1), members = in.add(a.members, nm);
  const auto pos = in.add(vw.pos, 3 * v), dir = in.add(vw.pos ? vw.dir : nullptr, 2 * v), centroid = in.add(vw.centroid, 3 * g), rg = in.add(vw.ring, 5 * ring);
  const auto vox = in.add(a.vox, 3 * n), group = in.add(vw.pos ? vw.group : nullptr, v);
  in.alloc();
  in.up(offsets, g + 1), in.up(members, nm), in.up(vox, 3 * n), in.up(pos, 3 * v), in.up(dir, 2 * v), in.up(group, v), in.up(centroid, 3 * g), in.up(rg, 5 * ring);
  const ViewIn vi{in.dev(vox), in.dev(offsets), in.dev(members), nullptr, a.n, G, NM, in.dev(pos), in.dev(dir), in.dev(group), V};
  const auto info = out.add(a.info, 1);
  const auto best_view = out.add(r.best_view, g);
  const auto best_count = out.add(r.best_count, g), n_in_view = out.add(r.n_in_view, v), n_visible = out.add(r.n_visible, v),
             cover_count = out.add(r.cover_count, n), first_view = out.add(r.first_view, n);
  const auto view_class = out.add(r.view_class, v);
  out.alloc();
  const fiesta_hip_view_result d{out.dev(view_class), out.dev(n_in_view), out.dev(n_visible), out.dev(cover_count),
                                 out.dev(first_view), out.dev(best_view), out.dev(best_count)};
  view_enqueue(st, S, vs, vi, in.dev(centroid), in.dev(rg), vw.n_ring, *a.sensor, d, out.dev(info));
  out.back(info, 1), out.back(view_class, v), out.back(n_in_view, v), out.back(n_visible, v), out.back(cover_count, n);
  out.back(first_view, n), out.back(best_view, g), out.back(best_count, g);
  FIESTA_HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace
}  // namespace fiesta
