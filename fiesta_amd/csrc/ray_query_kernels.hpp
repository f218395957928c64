// fiesta_amd/csrc/ray_query_kernels.hpp -- batched read-only ray queries: fiesta_hip_ray_query / _dev (include/fiesta_hip.h).
//
// A planner asks of a segment start -> end: which voxels would a sensor ray cross, where is the first occupied / never-observed /
// outside one, and how many unknown voxels lie before it (line of sight, the gain of a candidate view, an expected depth image).
// The walk is the ray cast's (ray_walk.hpp: dda_walk, unclipped and without the 1500-voxel exception) with the ray cast's rule for
// its last voxel: the end point's voxel floor(b) stands in for the traversal's last output (include/fiesta_hip.h, "the walk W").
//   k_ray_query<SRC>  one lane per ray, grid-stride.  A walk ends at its first blocking voxel, so most of a ray is never read:
//                     nothing is stored, the traversal hands every voxel (and "this is the last one") to the classification as it
//                     goes.  Per voxel: the centre and its map voxel in ray_visit_code's arithmetic (raycast.hip), then SRC:
//     DenseRaySource  (dense_read.hpp) the observed and the occupied bitmap; the last word pair (index, obs, occ) stays in registers,
//                     so a step along z re-reads nothing and a step along x or y costs one word pair
//     HashRaySource   (hash_read.hpp) the map-wide page lookup of the queries; the page address of the current tile stays in
//                     registers, a voxel costs its field word and, if observed, its occupancy word (kept while the row lasts)
// No atomics, no LDS, no scratch: every output is an integer or an f64 in a fixed operation order, the same for every launch shape.
#pragma once
#include <algorithm>
#include <cmath>

#include "../../include/fiesta_hip.h"
#include "common.hpp"
#include "planner.hpp"
#include "planner_args.hpp"
#include "ray_walk.hpp"

namespace fiesta {
namespace {  // (planner.hip alone includes this header; the namespace is part of the kernels' symbol names)

constexpr double kRayMaxCoord = 1073741824.0;  // 2^30: |start / resolution| and |end / resolution| stay below it
constexpr int64_t kRayMaxManhattan = 4095;     // voxel steps between the two ends
constexpr int kRayBlock = 256, kRayMaxBlocks = 2048;  // (8 waves per SIMD of 256 CUs; larger batches stride)
constexpr int32_t kRayNoVoxel = INT32_MIN;

// SRC: RayGeom g; Cache, fresh(), classify(walk voxel, map voxel of its centre, cache) -> FIESTA_HIP_RAY_* class
template <class SRC>
__global__ __launch_bounds__(kRayBlock) void k_ray_query(SRC src, const double *start, const double *end, int64_t n, int stop_mask,
                                                         fiesta_hip_ray_result r) {
  const double res = src.g.res;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    double s[3], a[3], b[3];
    bool ok = true;
    for (int c = 0; c < 3; ++c) {
      s[c] = start[3 * i + c];
      const double t = end[3 * i + c];
      a[c] = s[c] / res;
      b[c] = t / res;
      // (a non-finite component fails the comparison as well)
      ok = ok && fabs(s[c]) < (double)INFINITY && fabs(t) < (double)INFINITY && fabs(a[c]) < kRayMaxCoord && fabs(b[c]) < kRayMaxCoord;
    }
    int e0 = 0, e1 = 0, e2 = 0;
    if (ok) {
      e0 = (int)floor(b[0]), e1 = (int)floor(b[1]), e2 = (int)floor(b[2]);
      const int64_t m = llabs((int64_t)e0 - (int64_t)floor(a[0])) + llabs((int64_t)e1 - (int64_t)floor(a[1])) +
                        llabs((int64_t)e2 - (int64_t)floor(a[2]));
      ok = m <= kRayMaxManhattan;
    }
    int visited = -1, hit_index = -1, hit_class = 0, hv0 = kRayNoVoxel, hv1 = kRayNoVoxel, hv2 = kRayNoVoxel;
    int n_free = 0, n_occ = 0, n_unk = 0, n_out = 0;
    double hit_dist = __longlong_as_double(0x7FF8000000000000ll);
    if (ok) {
      typename SRC::Cache cache = SRC::fresh();
      auto visit = [&](int x, int y, int z, int k, bool last) -> bool {
        if (last) x = e0, y = e1, z = e2;  // the end point's voxel stands in for the traversal's last output
        const double p[3] = {(x + 0.5) * res, (y + 0.5) * res, (z + 0.5) * res};
        int v[3];
        for (int c = 0; c < 3; ++c)  // Pos2Vox, saturated (a map origin far from the ray)
          v[c] = (int)fmin(fmax(floor((p[c] - src.g.org[c]) / res), -2147483647.0), 2147483647.0);
        const int rr[3] = {x, y, z};
        const int cls = src.classify(rr, v, cache);
        visited = k + 1;
        if (cls & stop_mask) {
          hit_index = k, hit_class = cls, hv0 = v[0], hv1 = v[1], hv2 = v[2];
          const double q0 = p[0] - s[0], q1 = p[1] - s[1], q2 = p[2] - s[2];
          hit_dist = sqrt(q0 * q0 + q1 * q1 + q2 * q2);
          return true;
        }
        n_free += cls == FIESTA_HIP_RAY_FREE, n_occ += cls == FIESTA_HIP_RAY_OCCUPIED, n_unk += cls == FIESTA_HIP_RAY_UNKNOWN,
            n_out += cls == FIESTA_HIP_RAY_OUTSIDE;
        return false;
      };
      if (dda_walk<false, false>(a, b, nullptr, nullptr, visit) == 0) (void)visit(e0, e1, e2, 0, true);  // both ends in one voxel
    }
    if (r.n_visited) r.n_visited[i] = visited;
    if (r.hit_index) r.hit_index[i] = hit_index;
    if (r.hit_class) r.hit_class[i] = (uint8_t)hit_class;
    if (r.hit_vox) r.hit_vox[3 * i] = hv0, r.hit_vox[3 * i + 1] = hv1, r.hit_vox[3 * i + 2] = hv2;
    if (r.hit_dist) r.hit_dist[i] = hit_dist;
    if (r.counts) r.counts[4 * i] = n_free, r.counts[4 * i + 1] = n_occ, r.counts[4 * i + 2] = n_unk, r.counts[4 * i + 3] = n_out;
  }
}

// start / end / r: device pointers.  The grid follows from n alone; nothing is read back.
template <class SRC>
void ray_query_launch(hipStream_t st, const SRC &src, const double *start, const double *end, int64_t n, int stop_mask,
                      const fiesta_hip_ray_result &r) {
  const int blocks = (int)std::min<int64_t>((n + kRayBlock - 1) / kRayBlock, kRayMaxBlocks);
  hipLaunchKernelGGL(k_ray_query<SRC>, dim3(blocks), dim3(kRayBlock), 0, st, src, start, end, n, stop_mask, r);
  FIESTA_HIP_CHECK(hipGetLastError());
}

// Both variants of the call on a map's stream.  Host variant: the inputs are staged into S.in, the requested outputs come back
// through S.out, then the stream is synchronised.  Device variant: only enqueued.
template <class SRC>
void ray_query_run(hipStream_t st, PlannerScratch &S, const SRC &src, const RayArgs &a) {
  const fiesta_hip_ray_result &r = *a.res;
  if (a.dev) {
    ray_query_launch(st, src, a.start, a.end, a.n, a.stop_mask, r);
    return;
  }
  const size_t n = (size_t)a.n;
  Staging in{S.in, st}, out{S.out, st};
  const auto start = in.add(a.start, 3 * n), end = in.add(a.end, 3 * n);
  in.alloc(), in.up(start, 3 * n), in.up(end, 3 * n);
  const auto n_visited = out.add(r.n_visited, n), hit_index = out.add(r.hit_index, n), hit_vox = out.add(r.hit_vox, 3 * n),
             counts = out.add(r.counts, 4 * n);
  const auto hit_class = out.add(r.hit_class, n);
  const auto hit_dist = out.add(r.hit_dist, n);
  out.alloc();
  const fiesta_hip_ray_result d{out.dev(n_visited), out.dev(hit_index), out.dev(hit_class), out.dev(hit_vox), out.dev(hit_dist), out.dev(counts)};
  ray_query_launch(st, src, in.dev(start), in.dev(end), a.n, a.stop_mask, d);
  out.back(n_visited, n), out.back(hit_index, n), out.back(hit_class, n), out.back(hit_vox, 3 * n), out.back(hit_dist, n), out.back(counts, 4 * n);
  FIESTA_HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace
}  // namespace fiesta
