// fiesta_amd/csrc/ray_walk.hpp -- the reference's voxel traversal (src/raycast.cpp:56-158) as a device function, shared by the
// ray cast (raycast.hip: the frame's casting rays, k_raycast_one) and the read-only ray query (ray_query_kernels.hpp).
// All arithmetic is f64 in the reference's operation order; every user is compiled with -ffp-contract=off.
#pragma once
#include <cmath>
#include <type_traits>

#include "common.hpp"

namespace fiesta {

constexpr int kMaxRayVoxels = 1500;  // src/raycast.cpp:127-130
constexpr int kMaxRaySteps = 8192;   // the traversal's own loop bound

// what the walk needs of a map's geometry (a whole Geom as a kernel argument costs scalar registers the loop is short of)
struct RayGeom {
  double res, org[3];
};
inline RayGeom ray_geom(const Geom &g) { return RayGeom{g.res, {g.org[0], g.org[1], g.org[2]}}; }

__device__ inline int sgn_i(int v) { return v == 0 ? 0 : (v < 0 ? -1 : 1); }            // signum (:6-8)
__device__ inline double wrap1(double v) { return fmod(fmod(v, 1.0) + 1.0, 1.0); }      // mod (:10-12)
__device__ inline double first_crossing(double s, double ds) {                          // intbound (:14-23)
  if (ds < 0) {
    s = -s;
    ds = -ds;
  }
  return (1 - wrap1(s)) / ds;
}

// Amanatides-Woo traversal with the reference's arithmetic (src/raycast.cpp:56-158).  Returns the number of voxels the reference
// pushes, or -1 if it would exceed 1500 voxels (LIMIT; without it the exception of :127-130 is left out).  CLIP = false: no
// clipping box (lo / hi are not read) -- what min = -2^31, max = 2^31 would give, every int coordinate being inside.
// `emit` is called for every pushed voxel, in one of two forms:
//   emit(x, y, z, k)                  the ray cast's
//   bool emit(x, y, z, k, last)       last: the traversal ends with this voxel (it passed the end point's squared reach, reached the
//                                     end voxel, or the loop bound ran out); returning true ends the traversal here
template <bool LIMIT = true, bool CLIP = true, typename Emit>
__device__ inline int dda_walk(const double *a, const double *b, const double *lo, const double *hi, Emit emit) {
  int c[3] = {(int)floor(a[0]), (int)floor(a[1]), (int)floor(a[2])};
  const int e[3] = {(int)floor(b[0]), (int)floor(b[1]), (int)floor(b[2])};
  const double r0 = b[0] - a[0], r1 = b[1] - a[1], r2 = b[2] - a[2];
  const double reach2 = r0 * r0 + r1 * r1 + r2 * r2;
  double tmax[3], tstep[3];
  int step[3];
  for (int i = 0; i < 3; ++i) {
    const double delta = e[i] - c[i];  // NB: integer voxel delta, not the true ray direction (:89-91)
    step[i] = sgn_i((int)delta);
    tmax[i] = first_crossing(a[i], delta);
    tstep[i] = ((double)step[i]) / delta;
  }
  if (step[0] == 0 && step[1] == 0 && step[2] == 0) return 0;
  int count = 0;
  for (int guard = 0; guard < kMaxRaySteps; ++guard) {
    const bool at_end = c[0] == e[0] && c[1] == e[1] && c[2] == e[2];
    if (!CLIP || (c[0] >= lo[0] && c[0] < hi[0] && c[1] >= lo[1] && c[1] < hi[1] && c[2] >= lo[2] && c[2] < hi[2])) {
      const double q0 = c[0] - a[0], q1 = c[1] - a[1], q2 = c[2] - a[2];
      const bool past = q0 * q0 + q1 * q1 + q2 * q2 > reach2;
      if constexpr (std::is_invocable_v<Emit, int, int, int, int>) {
        emit(c[0], c[1], c[2], count);
        ++count;
      } else {
        const bool stop = emit(c[0], c[1], c[2], count, past || at_end || guard == kMaxRaySteps - 1);
        ++count;
        if (stop) return count;
      }
      if (past) return count;
      if (LIMIT && count > kMaxRayVoxels) return -1;
    }
    if (at_end) break;
    int ax;  // strict '<' tie rules (:139-157)
    if (tmax[0] < tmax[1])
      ax = (tmax[0] < tmax[2]) ? 0 : 2;
    else
      ax = (tmax[1] < tmax[2]) ? 1 : 2;
    c[ax] += step[ax];
    tmax[ax] += tstep[ax];
  }
  return count;
}

// PosInMap (src/ESDFMap.cpp:46-52) of the array build
__device__ inline bool ray_pos_in_map(const Geom &g, const double *p) {
  return !(p[0] < g.lo[0] || p[1] < g.lo[1] || p[2] < g.lo[2] || p[0] > g.hi[0] || p[1] > g.hi[1] || p[2] > g.hi[2]);
}

}  // namespace fiesta
