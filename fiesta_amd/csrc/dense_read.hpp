// fiesta_amd/csrc/dense_read.hpp -- what can be read of a dense map: the arithmetic of its queries, the sources and evaluators the
// planner kernels take, and DenseView, the plain view DenseMap::planner_view() hands to the planner calls of planner.hip.
// dense_map.hip includes it for the point-query kernels and the host brick cache.  No kernel is defined here.
#pragma once
#include <algorithm>
#include <cmath>

#include "../../include/fiesta_hip.h"
#include "common.hpp"
#include "planner.hpp"
#include "ray_walk.hpp"

namespace fiesta {

// The arithmetic of the queries is written once, over any SOURCE of voxel words: the batch kernels read the field in HBM, the
// scalar host calls of the drop-in class (one position per call: fiesta::ESDFMap::GetDistance & co., include/fiesta/ESDFMap.h)
// read a host-side cache of 16^3-voxel bricks (DenseMap::HostBricks, dense_map.hip) -- same code, same -ffp-contract=off, same bits.
__host__ __device__ inline double word_distance(const Geom &g, vox_t w, int x, int y, int z) {
  // GetDistance(Vector3i) (src/ESDFMap.cpp:477-479): unobserved (-10000) reads as +10000
  if (w & kNoCoc) return (double)FIESTA_HIP_INFINITY;
  const int32_t d2 = dist2(g.wrap, x + g.gx0, y + g.gy0, z + g.gz0, w);
  return sqrt((double)d2) * g.res;  // Dist (:122-124)
}
struct FieldWords {  // the field itself
  const Geom &g;
  const vox_t *coc;
  __device__ inline vox_t operator()(int x, int y, int z) const { return coc[g.idx(x, y, z)]; }
};
template <class Words>
__host__ __device__ inline double vox_distance(const Geom &g, Words &wd, int x, int y, int z) {
  if (!g.in_grid(x, y, z)) return (double)FIESTA_HIP_INFINITY;  // the reference reads out of bounds here
  return word_distance(g, wd(x, y, z) & ~kAct, x, y, z);
}
__host__ __device__ inline bool pos_in_map(const Geom &g, double px, double py, double pz) {  // PosInMap (:46-61)
  return !(px < g.lo[0] || py < g.lo[1] || pz < g.lo[2] || px > g.hi[0] || py > g.hi[1] || pz > g.hi[2]);
}
template <class Words>
__host__ __device__ inline double query_dist_pos(const Geom &g, Words &wd, double px, double py, double pz) {  // (:467-475)
  if (!pos_in_map(g, px, py, pz)) return (double)FIESTA_HIP_UNDEFINED;
  return vox_distance(g, wd, (int)floor((px - g.org[0]) / g.res) - g.gx0, (int)floor((py - g.org[1]) / g.res) - g.gy0,
                      (int)floor((pz - g.org[2]) / g.res) - g.gz0);
}
// GetDistWithGradTrilinear (src/ESDFMap.cpp:481-540), same operation order in f64 (compiled with -ffp-contract=off so no
// FMA contraction changes the last bit).  grad: three doubles or null.
template <class Words>
__host__ __device__ inline double query_trilinear(const Geom &g, Words &wd, const double *p, double *grad) {
  if (!pos_in_map(g, p[0], p[1], p[2])) {
    if (grad) grad[0] = grad[1] = grad[2] = 0;
    return -1;
  }
  int b[3];
  double f[3];
  for (int k = 0; k < 3; ++k) {
    const double pm = p[k] - 0.5 * g.res * 1.0;
    b[k] = (int)floor((pm - g.org[k]) / g.res);
    const double c = (b[k] + 0.5) * g.res + g.org[k];
    f[k] = (p[k] - c) * g.res_inv;
  }
  double v[2][2][2];
  for (int ix = 0; ix < 2; ++ix)
    for (int iy = 0; iy < 2; ++iy)
      for (int iz = 0; iz < 2; ++iz)
        v[ix][iy][iz] = vox_distance(g, wd, b[0] + ix - g.gx0, b[1] + iy - g.gy0, b[2] + iz - g.gz0);
  const double v00 = (1 - f[0]) * v[0][0][0] + f[0] * v[1][0][0];
  const double v01 = (1 - f[0]) * v[0][0][1] + f[0] * v[1][0][1];
  const double v10 = (1 - f[0]) * v[0][1][0] + f[0] * v[1][1][0];
  const double v11 = (1 - f[0]) * v[0][1][1] + f[0] * v[1][1][1];
  const double v0 = (1 - f[1]) * v00 + f[1] * v10;
  const double v1 = (1 - f[1]) * v01 + f[1] * v11;
  if (grad) {
    grad[2] = (v1 - v0) * g.res_inv;
    grad[1] = ((1 - f[2]) * (v10 - v00) + f[2] * (v11 - v01)) * g.res_inv;
    double gx = (1 - f[2]) * (1 - f[1]) * (v[1][0][0] - v[0][0][0]);
    gx += (1 - f[2]) * f[1] * (v[1][1][0] - v[0][1][0]);
    gx += f[2] * (1 - f[1]) * (v[1][0][1] - v[0][0][1]);
    gx += f[2] * f[1] * (v[1][1][1] - v[0][1][1]);
    grad[0] = gx * g.res_inv;
  }
  return (1 - f[2]) * v0 + f[2] * v1;
}

// the sample evaluator of the path kernels (path_kernels.hpp): k_query_trilinear's arithmetic on the field itself
struct DensePathEval {
  Geom g;
  const vox_t *coc;
  __device__ double operator()(const double *p, double *grad) const {
    FieldWords wd{g, coc};
    return query_trilinear(g, wd, p, grad);
  }
};
// the clearance filter of the frontier kernel (frontier_kernels.hpp): GetDistance(Vector3i) on the field itself, local coordinates
struct DenseFrontierDist {
  Geom g;
  const vox_t *coc;
  __device__ double operator()(int x, int y, int z) const {
    FieldWords wd{g, coc};
    return vox_distance(g, wd, x, y, z);
  }
};
// the map side of the reachability flood (reach_kernels.hpp: k_reach_mask), local array coordinates: 32 voxels of the two bitmaps
// from any z (two words and a funnel shift when z0 is no multiple of 32; past the array: zero) and the frontier filter's distance
struct DenseReachSource {
  Geom g;
  const uint32_t *obs, *occ;
  const vox_t *coc;
  __device__ void row(int x, int y, int z0, uint32_t &o, uint32_t &c) const {
    const int64_t wi = g.bitword(x, y, z0);
    const int s = z0 & 31;
    const uint32_t o0 = obs[wi], c0 = occ[wi];
    uint32_t o1 = 0, c1 = 0;
    if (s && (z0 >> 5) + 1 < g.nzw) o1 = obs[wi + 1], c1 = occ[wi + 1];
    o = reach_funnel(o0, o1, s), c = reach_funnel(c0, c1, s);
  }
  __device__ double operator()(int x, int y, int z) const {
    FieldWords wd{g, coc};
    return vox_distance(g, wd, x, y, z);
  }
};

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

// the voxel source of the ray query (ray_query_kernels.hpp): the observed and the occupied bitmap; the last word pair (index, obs,
// occ) stays in registers
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

// A dense map as the planner calls see it: its geometry and the device arrays the sources read.  The host members are the
// store's side of a call: the sources, how a caller's box becomes the kernels' box, and what turns that box back into map voxels.
struct DenseView {
  Geom g;
  const vox_t *coc;
  const uint32_t *obs, *occ;
  int off[3];  // the sources take local array coordinates: map voxel minus the array's first voxel

  DensePathEval path_eval() const { return DensePathEval{g, coc}; }
  DenseFrontierDist frontier() const { return DenseFrontierDist{g, coc}; }
  const vox_t *field() const { return coc; }  // the skeleton kernel's word source: the field itself, z fastest (Geom::idx)
  DenseReachSource reach_source() const { return DenseReachSource{g, obs, occ, coc}; }
  DenseRaySource ray_source() const { return DenseRaySource(g, obs, occ); }
  // a caller's box (null: everything) in local array coordinates, intersected with the array; false: nothing is left
  bool clip_box(const int32_t *lo, const int32_t *hi, int64_t blo[3], int64_t bhi[3]) const {
    const int dims[3] = {g.nx, g.ny, g.nz};
    bool any = true;
    for (int c = 0; c < 3; ++c) {
      blo[c] = lo ? std::max<int64_t>((int64_t)lo[c] - off[c], 0) : 0;
      bhi[c] = hi ? std::min<int64_t>((int64_t)hi[c] - off[c], dims[c] - 1) : dims[c] - 1;
      any = any && blo[c] <= bhi[c];
    }
    return any;
  }
  // the reach calls' clipped box, checked before anything is launched; empty: blo[0] > bhi[0].  The padding bits of a row's last
  // bitmap word lie past the clipped box and are masked there.
  void reach_box(const int32_t *lo, const int32_t *hi, int64_t blo[3], int64_t bhi[3]) const {
    const bool empty = !clip_box(lo, hi, blo, bhi);
    if (empty) blo[0] = 1, bhi[0] = 0;
    if (!empty && (bhi[0] - blo[0] + 1) * (bhi[1] - blo[1] + 1) * (bhi[2] - blo[2] + 1) > kReachMaxVoxels)
      throw Error(FIESTA_HIP_ERR_INVALID, "reach: the clipped box holds more than 2^28 voxels");
  }
  // the corridor calls' window in MAP voxel coordinates: the caller's box clipped to the array (both null: the whole array); empty: wlo[0] > whi[0]
  void corridor_window(const int32_t *lo, const int32_t *hi, int wlo[3], int whi[3]) const {
    int64_t blo[3], bhi[3];
    const bool any = clip_box(lo, hi, blo, bhi);
    for (int c = 0; c < 3; ++c) wlo[c] = (int)(blo[c] + off[c]), whi[c] = (int)(bhi[c] + off[c]);
    if (!any) wlo[0] = 1, whi[0] = 0;
  }
};

}  // namespace fiesta
