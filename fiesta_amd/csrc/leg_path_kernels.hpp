// fiesta_amd/csrc/leg_path_kernels.hpp -- the legs of a tour, out of the reach matrix's floods: fiesta_hip_leg_paths / _dev
// (include/fiesta_hip.h).
//
// fiesta_hip_reach_matrix has flooded the box from every site, and while all sources fitted ONE batch its cost planes still lie in the
// map's scratch (ReachMatrixScratch: the RETAINED batch, plane s = the flood of source s).  A leg from site `from` to a target is
// fiesta_hip_reach_paths' path for that target on plane `from`: the rule is not restated here -- the kernels build a ReachPathField whose
// cost points at the leg's plane and call reach_path_start / reach_path_wave / reach_path_store of reach_path_kernels.hpp.
//   k_leg_path_count<CONN>  per leg: status (BAD_INDEX, NO_SOURCE, then reach_paths' own), number of moves, the plane's cost at the target,
//                           number of waypoints (into offsets[k + 1])
//   k_reach_path_scan       (reach_path_kernels.hpp, as it is) offsets[1 .. n] -> running totals
//   k_leg_path_write<CONN>  redoes the rule and stores the waypoints below the capacity, source first, target last
// Shape: ONE WAVE PER LEG, in a work-group of its own.  A batch is the legs of a tour -- tens to a few hundred -- and each is a serial
// descent of up to hundreds of dependent loads: what counts is how many CUs work at once, and 63 work-groups of one wave occupy 63
// CUs where reach_paths' groups of four waves (shaped for tens of thousands of targets) would occupy 16.  Both modes take the wave
// form: raw mode is max_span = 1, which passes no visibility test at all (a step is one load per lane and a ballot).
// No atomics, no LDS, no scratch; every store is a plain store of one lane.
#pragma once
#include <algorithm>
#include <climits>

#include "../../include/fiesta_hip.h"
#include "common.hpp"
#include "planner.hpp"
#include "planner_args.hpp"
#include "reach_path_kernels.hpp"

namespace fiesta {
namespace {  // (planner.hip alone includes this header; the namespace is part of the kernels' symbol names)

#ifndef FIESTA_LEG_PATH_WAVES
#define FIESTA_LEG_PATH_WAVES 1  // waves, and so legs, per work-group (a build-time knob for tools/leg_paths_bench.py --lib: DESIGN.md 6o)
#endif
constexpr int kLegPathWaves = FIESTA_LEG_PATH_WAVES;
constexpr int64_t kLegPathMaxGroups = 1 << 20;  // work-groups of one launch, a leg per wave; more legs: more launches

struct LegPathBatch {  // the retained batch, device pointers
  const int32_t *planes;  // n_sources planes of nvox costs
  int64_t nvox;
  const int32_t *sites;   // n_sources x 3 map voxels
  const int32_t *status;  // FIESTA_HIP_REACH_SITE_* per source
  int n_sources;
};
struct LegPathIn {  // device pointers; to or to_vox is null
  const int32_t *from, *to, *to_vox;
  int64_t n;
};

// Leg k: BAD_INDEX, NO_SOURCE, or -1 and the leg's field (f.cost = its source's plane) and target (entry p of tg).  Wave-uniform.
__device__ inline int leg_path_resolve(const LegPathBatch &b, const LegPathIn &in, int64_t k, ReachPathField &f, const int32_t *&tg, int64_t &p) {
  const int s = in.from[k], t = in.to ? in.to[k] : 0;
  if ((unsigned)s >= (unsigned)b.n_sources || (unsigned)t >= (unsigned)b.n_sources) return FIESTA_HIP_LEG_BAD_INDEX;
  if (b.status[s] != FIESTA_HIP_REACH_SITE_OK) return FIESTA_HIP_LEG_NO_SOURCE;
  f.cost = b.planes + (int64_t)s * b.nvox;
  tg = in.to ? b.sites : in.to_vox, p = in.to ? (int64_t)t : k;
  return -1;
}

// count pass: offsets[k + 1] = number of waypoints of leg k (the scan turns them into totals); status, n_moves and cost
template <int CONN>
__global__ __launch_bounds__(64 * kLegPathWaves) void k_leg_path_count(ReachPathField f, LegPathBatch b, LegPathIn in, ReachPathOut o, int32_t *cost,
                                                                       int max_span, int64_t k0) {
  const int64_t k = k0 + (int64_t)blockIdx.x * kLegPathWaves + (threadIdx.x >> 6);  // (the launch has exactly one wave per leg ...
  if (k >= in.n) return;                                                            //  ... but for the last group's spare waves)
  const int32_t *tg = nullptr;
  int64_t p = 0;
  int L = -1, cnt = 0, c = -1;
  int st = leg_path_resolve(b, in, k, f, tg, p);
  if (st < 0) {
    int x = 0, y = 0, z = 0;
    if (reach_path_start(f, tg, p, x, y, z, c) == FIESTA_HIP_REACH_PATH_OUTSIDE) c = -1;  // (else: the plane at the target voxel)
    st = reach_path_wave<CONN, false>(f, o, tg, p, max_span, 0, 0, L, cnt);
  }
  if (st != FIESTA_HIP_REACH_PATH_OK) L = -1, cnt = 0;
  if ((threadIdx.x & 63) == 0) {
    o.offsets[k + 1] = cnt;
    if (o.status) o.status[k] = st;
    if (o.n_moves) o.n_moves[k] = L;
    if (cost) cost[k] = c;
  }
}

template <int CONN>
__global__ __launch_bounds__(64 * kLegPathWaves) void k_leg_path_write(ReachPathField f, LegPathBatch b, LegPathIn in, ReachPathOut o, int max_span,
                                                                       int64_t k0) {
  const int64_t k = k0 + (int64_t)blockIdx.x * kLegPathWaves + (threadIdx.x >> 6);
  if (k >= in.n) return;
  const int64_t first = o.offsets[k], count = o.offsets[k + 1] - first;
  if (count <= 0 || first >= o.capacity) return;  // no path, or all of it beyond the capacity
  const int32_t *tg = nullptr;
  int64_t p = 0;
  if (leg_path_resolve(b, in, k, f, tg, p) >= 0) return;  // (the indices changed between the two passes)
  int L, cnt;
  (void)reach_path_wave<CONN, true>(f, o, tg, p, max_span, first, count, L, cnt);
}

inline void leg_path_launch(hipStream_t st, const ReachPathField &f, const LegPathBatch &b, const LegPathIn &in, const ReachPathOut &o, int32_t *cost,
                            int connectivity, int max_span, bool count) {
  const dim3 block(64 * kLegPathWaves);
  for (int64_t k0 = 0; k0 < in.n; k0 += kLegPathMaxGroups * kLegPathWaves) {  // (one launch for any batch a planner has)
    const dim3 groups((unsigned)std::min<int64_t>((in.n - k0 + kLegPathWaves - 1) / kLegPathWaves, kLegPathMaxGroups));
    if (count) {
      if (connectivity == 6)
        hipLaunchKernelGGL(k_leg_path_count<6>, groups, block, 0, st, f, b, in, o, cost, max_span, k0);
      else
        hipLaunchKernelGGL(k_leg_path_count<26>, groups, block, 0, st, f, b, in, o, cost, max_span, k0);
    } else {
      if (connectivity == 6)
        hipLaunchKernelGGL(k_leg_path_write<6>, groups, block, 0, st, f, b, in, o, max_span, k0);
      else
        hipLaunchKernelGGL(k_leg_path_write<26>, groups, block, 0, st, f, b, in, o, max_span, k0);
    }
    FIESTA_HIP_CHECK(hipGetLastError());
  }
}

// Both variants of the call on a map's stream; res / org: the map's resolution and origin -- nothing else of a map is read, so both
// stores share this function.  The device variant only enqueues (count, scan, write).  The host variant stages the legs through P.in
// and the outputs through P.out, reads the totals back between the count and the write pass -- so that it stages min(total,
// capacity) waypoints, not the capacity -- and synchronises.  The retained batch is read, never written.
inline void leg_paths_run(hipStream_t st, PlannerScratch &P, double res, const double *org, const LegPathArgs &a) {
  const ReachMatrixScratch &S = P.reach_matrix;
  if (!S.batch_valid)
    throw Error(FIESTA_HIP_ERR_STATE, S.batch_why == ReachMatrixScratch::kNoCallYet     ? "leg_paths: the map retains no batch (no reach_matrix call yet)"
                                      : S.batch_why == ReachMatrixScratch::kManyBatches ? "leg_paths: the map retains no batch (the last reach_matrix call "
                                                                                          "ran more than one batch: info->batches)"
                                                                                        : "leg_paths: the map retains no batch (the last reach_matrix call had "
                                                                                          "no source or an empty box, or it failed)");
  if (a.info) {
    fiesta_hip_leg_paths_info &I = *a.info;
    I = fiesta_hip_leg_paths_info{};
    for (int c = 0; c < 3; ++c) I.box_lo[c] = S.batch_lo[c], I.box_hi[c] = S.batch_hi[c];
    I.connectivity = S.batch_connectivity, I.n_sources = S.batch_sources;
  }
  const fiesta_hip_leg_paths_result &r = *a.res;
  ReachPathField f{};
  f.ox = S.batch_lo[0], f.oy = S.batch_lo[1], f.oz = S.batch_lo[2];
  f.ex = S.batch_hi[0] - S.batch_lo[0] + 1, f.ey = S.batch_hi[1] - S.batch_lo[1] + 1, f.ez = S.batch_hi[2] - S.batch_lo[2] + 1;
  f.res = res, f.org[0] = org[0], f.org[1] = org[1], f.org[2] = org[2];
  const LegPathBatch b{S.planes.p, (int64_t)f.ex * f.ey * f.ez, S.sites.p, S.status.p, (int)S.batch_sources};
  const int max_span = (a.flags & FIESTA_HIP_REACH_PATHS_SHORTCUT) ? a.max_span : 1;  // raw: every voxel of the descent is an anchor
  const int conn = S.batch_connectivity;
  const int64_t n = a.n_legs;
  if (a.dev) {
    const LegPathIn in{a.from, a.to, a.to_vox, n};
    const ReachPathOut o{r.offsets, r.waypoints_vox, r.waypoints_pos, r.status, r.n_moves, a.capacity};
    if (n > 0) leg_path_launch(st, f, b, in, o, r.cost, conn, max_span, true);
    hipLaunchKernelGGL(k_reach_path_scan, dim3(1), dim3(256), 0, st, r.offsets, n);
    FIESTA_HIP_CHECK(hipGetLastError());
    if (n > 0 && a.capacity > 0 && (r.waypoints_vox || r.waypoints_pos)) leg_path_launch(st, f, b, in, o, nullptr, conn, max_span, false);
    return;
  }
  if (n == 0) {
    r.offsets[0] = 0;
    return;
  }
  const size_t cnt = (size_t)n;
  Staging in{P.in, st}, out{P.out, st};
  const auto from = in.add(a.from, cnt), to = in.add(a.to, cnt), to_vox = in.add(a.to_vox, 3 * cnt);
  in.alloc(), in.up(from, cnt), in.up(to, cnt), in.up(to_vox, 3 * cnt);
  const LegPathIn legs{in.dev(from), in.dev(to), in.dev(to_vox), n};
  // offsets, status, n_moves and cost; the waypoints follow once their number is known
  const auto offsets = out.add(r.offsets, cnt + 1);
  const auto status = out.add(r.status, cnt), n_moves = out.add(r.n_moves, cnt), cost = out.add(r.cost, cnt);
  const size_t head = out.end;
  out.alloc();
  ReachPathOut o{out.dev(offsets), nullptr, nullptr, out.dev(status), out.dev(n_moves), 0};
  leg_path_launch(st, f, b, legs, o, out.dev(cost), conn, max_span, true);
  hipLaunchKernelGGL(k_reach_path_scan, dim3(1), dim3(256), 0, st, o.offsets, n);
  FIESTA_HIP_CHECK(hipGetLastError());
  out.back(offsets, cnt + 1), out.back(status, cnt), out.back(n_moves, cnt), out.back(cost, cnt);
  FIESTA_HIP_CHECK(hipStreamSynchronize(st));
  const int64_t w = std::min<int64_t>(r.offsets[n], a.capacity);
  if (w <= 0 || (!r.waypoints_vox && !r.waypoints_pos)) return;
  const auto pos = out.add(r.waypoints_pos, 3 * (size_t)w);
  const auto vox = out.add(r.waypoints_vox, 3 * (size_t)w);
  out.alloc(head);  // (the buffer may move; the scanned offsets are kept: the write pass reads them)
  o = ReachPathOut{out.dev(offsets), out.dev(vox), out.dev(pos), nullptr, nullptr, w};
  leg_path_launch(st, f, b, legs, o, nullptr, conn, max_span, false);
  out.back(pos, 3 * (size_t)w), out.back(vox, 3 * (size_t)w);
  FIESTA_HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace
}  // namespace fiesta
