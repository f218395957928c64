// fiesta_amd/csrc/ray_query_kernels.hpp -- batched read-only ray queries: fiesta_hip_ray_query / _dev (include/fiesta_hip.h).
//
// A planner asks of a segment start -> end: which voxels would a sensor ray cross, where is the first occupied / never-observed /
// outside one, and how many unknown voxels lie before it (line of sight, the gain of a candidate view, an expected depth image).
// The walk is the ray cast's (ray_walk.hpp: dda_walk, unclipped and without the 1500-voxel exception) with the ray cast's rule for
// its last voxel: the end point's voxel floor(b) stands in for the traversal's last output (include/fiesta_hip.h, "the walk W").
//   k_ray_query<SRC>  one lane per ray, grid-stride.  A walk ends at its first blocking voxel, so most of a ray is never read:
//                     nothing is stored, the traversal hands every voxel (and "this is the last one") to the classification as it
//                     goes.  Per voxel: the centre and its map voxel in ray_visit_code's arithmetic (raycast.hip), then SRC:
//     DenseRaySource  the observed and the occupied bitmap; the last word pair (index, obs, occ) stays in registers, so a step along
//                     z re-reads nothing and a step along x or y costs one word pair
//     HashRaySource   (hash_map.hip) the map-wide page lookup of the queries; the page address of the current tile stays in
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
namespace {  // (this header is included by two translation units)

constexpr double kRayMaxCoord = 1073741824.0;  // 2^30: |start / resolution| and |end / resolution| stay below it
constexpr int64_t kRayMaxManhattan = 4095;     // voxel steps between the two ends
constexpr int kRayBlock = 256, kRayMaxBlocks = 2048;  // (8 waves per SIMD of 256 CUs; larger batches stride)
constexpr int32_t kRayNoVoxel = INT32_MIN;

// what the walk needs of a map's geometry (a whole Geom as a kernel argument costs scalar registers the loop is short of)
struct RayGeom {
  double res, org[3];
};
inline RayGeom ray_geom(const Geom &g) { return RayGeom{g.res, {g.org[0], g.org[1], g.org[2]}}; }

// PosInMap of a voxel CENTRE as a test on the walk voxel r itself: the centre (r + 0.5) * res never decreases as r grows (the sum is
// exact below 2^31, the product is rounded once), so "centre >= bound" holds from some r on.  That r, by bisection over the range
// a valid ray can reach (strict: "centre > bound"); evaluated with the kernel's own arithmetic (-ffp-contract=off on the host too).
inline int ray_first_centre(double bound, double res, bool strict) {
  int64_t lo = -(1ll << 30) - 2, hi = (1ll << 30) + 2;  // answer in (lo, hi]: hi if no voxel in between qualifies
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    const double p = ((double)mid + 0.5) * res;
    if (strict ? p > bound : p >= bound)
      hi = mid;
    else
      lo = mid;
  }
  return (int)hi;
}

struct DenseRaySource {
  RayGeom g;
  int rlo[3], rhi[3];  // PosInMap(centre of walk voxel r) <=> rlo[c] <= r[c] <= rhi[c] (min_range_ / max_range_)
  int nx, ny, nz, nzw, gx0, gy0, gz0;
  const uint32_t *obs, *occ;
  DenseRaySource(const Geom &G, const uint32_t *obsbits, const uint32_t *occbits)
      : g(ray_geom(G)), nx(G.nx), ny(G.ny), nz(G.nz), nzw(G.nzw), gx0(G.gx0), gy0(G.gy0), gz0(G.gz0), obs(obsbits), occ(occbits) {
    for (int c = 0; c < 3; ++c) rlo[c] = ray_first_centre(G.lo[c], G.res, false), rhi[c] = ray_first_centre(G.hi[c], G.res, true) - 1;
  }
  struct Cache {
    int64_t w;
    uint32_t obs, occ;
  };
  __device__ static Cache fresh() { return Cache{-1, 0u, 0u}; }
  // r: the walk voxel, v: its centre's map voxel
  __device__ int classify(const int *r, const int *v, Cache &c) const {
    if (r[0] < rlo[0] || r[1] < rlo[1] || r[2] < rlo[2] || r[0] > rhi[0] || r[1] > rhi[1] || r[2] > rhi[2]) return FIESTA_HIP_RAY_OUTSIDE;  // PosInMap
    const int64_t x = (int64_t)v[0] - gx0, y = (int64_t)v[1] - gy0, z = (int64_t)v[2] - gz0;
    if ((uint64_t)x >= (uint64_t)nx || (uint64_t)y >= (uint64_t)ny || (uint64_t)z >= (uint64_t)nz) return FIESTA_HIP_RAY_OUTSIDE;
    const int64_t w = (x * ny + y) * nzw + (z >> 5);  // Geom::bitword
    if (w != c.w) c.w = w, c.obs = obs[w], c.occ = occ[w];
    const int bit = (int)z & 31;
    if (!((c.obs >> bit) & 1u)) return FIESTA_HIP_RAY_UNKNOWN;
    return ((c.occ >> bit) & 1u) ? FIESTA_HIP_RAY_OCCUPIED : FIESTA_HIP_RAY_FREE;
  }
};

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
