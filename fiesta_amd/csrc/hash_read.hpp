// fiesta_amd/csrc/hash_read.hpp -- what can be read of a hash-block map: the lookup and the arithmetic of its queries, the sources
// and evaluators the planner kernels take, and HashView, the plain view HashMap::planner_view() hands to the planner
// calls of planner.hip.  hash_map.hip includes it for the point-query kernels and the host brick cache.  No kernel is defined here.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>

#include "../../include/fiesta_hip.h"
#include "common.hpp"
#include "hash_map.hpp"
#include "planner.hpp"
#include "ray_walk.hpp"

namespace fiesta {

constexpr int kWin = HashMap::kWin;
constexpr int kNTY = HashMap::kNTY, kNTZ = HashMap::kNTZ;
constexpr int kPageVox = HashMap::kPageVox;
// a caller's voxel coordinate or range bound clamped to +-2^30 (map coordinates lie well inside): kernels' differences stay in range
inline int clamp30(int64_t v) { return (int)std::min<int64_t>(std::max<int64_t>(v, -(1ll << 30)), 1ll << 30); }

__device__ inline int tile_id(int x, int y, int z) { return ((x >> 4) * kNTY + (y >> 4)) * kNTZ + (z >> 5); }
__device__ inline bool in_win(int x, int y, int z) {
  return (unsigned)x < (unsigned)kWin && (unsigned)y < (unsigned)kWin && (unsigned)z < (unsigned)kWin;
}
// pool address of window voxel (x,y,z); -1 if its page is not allocated
__device__ inline int64_t vaddr(const int32_t *dir, int x, int y, int z) {
  const int32_t p = dir[tile_id(x, y, z)];
  return p < 0 ? -1 : (int64_t)p * kPageVox + (((x & 15) * 16 + (y & 15)) * 32 + (z & 31));
}
__device__ inline bool hbit(const uint32_t *bits, int64_t addr) { return (bits[addr >> 5] >> (addr & 31)) & 1u; }
// The window MOVES (HashMap::ensure_window): window voxel (0,0,0) is map voxel (g.gx0, g.gy0, g.gz0), a multiple of the
// tile size.  Closest-obstacle ids are therefore stored as MAP coordinates modulo 1024 and decoded relative to the voxel
// that holds them (common.hpp: coc_offset with wrap; reach 512 voxels) -- they stay valid when the window moves.
__device__ inline int32_t h_dist2(const Geom &g, int x, int y, int z, vox_t w) {
  return dist2(1, x + g.gx0, y + g.gy0, z + g.gz0, w);
}

// ---- queries (src/ESDFMap.cpp:452-540); an unallocated voxel reads like a freshly allocated one ----
// The reference's hash map answers for ANY voxel it ever allocated (:732-765).  Inside the window a lookup is one load of
// the dense directory; outside it -- pages that are parked -- a query goes through the MAP-WIDE page table: every page's
// tile in map coordinates as a sorted 64-bit key (a few thousand entries: a binary search), so that a planner may ask for
// a goal far from the sensor.  A parked page answers with the field it held when the window left it.
struct PageTable {  // every page's tile in MAP coordinates, sorted: what a query outside the window searches (h_lookup)
  const unsigned long long *keys;  // (tx + 2^20) << 42 | (ty + 2^20) << 21 | (tz + 2^20)
  const int32_t *pages;
  int n;
};
__host__ __device__ inline unsigned long long tile_key(int tx, int ty, int tz) {
  return ((unsigned long long)(uint32_t)(tx + (1 << 20)) << 42) | ((unsigned long long)(uint32_t)(ty + (1 << 20)) << 21) |
         (unsigned long long)(uint32_t)(tz + (1 << 20));
}
// pool address of WINDOW voxel (x, y, z), which may lie outside the window; -1: no page anywhere holds it
__device__ inline int64_t h_lookup(const Geom &g, const int32_t *dir, const PageTable &tab, int x, int y, int z) {
  if (in_win(x, y, z)) return vaddr(dir, x, y, z);
  const int vx = x + g.gx0, vy = y + g.gy0, vz = z + g.gz0;  // map voxel; the window origin is a whole number of tiles
  const unsigned long long key = tile_key(vx >> 4, vy >> 4, vz >> 5);
  int lo = 0, hi = tab.n - 1;
  while (lo <= hi) {
    const int mid = (lo + hi) >> 1;
    const unsigned long long k = tab.keys[mid];
    if (k == key) return (int64_t)tab.pages[mid] * kPageVox + (((vx & 15) * 16 + (vy & 15)) * 32 + (vz & 31));
    if (k < key)
      lo = mid + 1;
    else
      hi = mid - 1;
  }
  return -1;
}
__device__ inline double h_distance(const Geom &g, const int32_t *dir, const PageTable &tab, const vox_t *coc, int x, int y, int z) {
  const int64_t a = h_lookup(g, dir, tab, x, y, z);
  if (a < 0) return (double)FIESTA_HIP_INFINITY;
  const vox_t w = coc[a] & ~kAct;
  if (w & kNoCoc) return (double)FIESTA_HIP_INFINITY;
  return sqrt((double)h_dist2(g, x, y, z, w)) * g.res;
}
// GetDistWithGradTrilinear (src/ESDFMap.cpp:481-540), f64 in the reference's operation order -- written once over a source of
// corner distances D(map voxel x, y, z), compiled for the device (the batch kernel) and for the host (scalar calls from the brick
// cache): the two are bit-equal
template <class D>
__host__ __device__ inline double h_trilinear(const Geom &g, D &&corner, const double *p, double *grad) {
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
      for (int iz = 0; iz < 2; ++iz) v[ix][iy][iz] = corner(b[0] + ix, b[1] + iy, b[2] + iz);
  const double v00 = (1 - f[0]) * v[0][0][0] + f[0] * v[1][0][0];
  const double v01 = (1 - f[0]) * v[0][0][1] + f[0] * v[1][0][1];
  const double v10 = (1 - f[0]) * v[0][1][0] + f[0] * v[1][1][0];
  const double v11 = (1 - f[0]) * v[0][1][1] + f[0] * v[1][1][1];
  const double v0 = (1 - f[1]) * v00 + f[1] * v10;
  const double v1 = (1 - f[1]) * v01 + f[1] * v11;
  const double d = (1 - f[2]) * v0 + f[2] * v1;
  if (grad) {
    grad[2] = (v1 - v0) * g.res_inv;
    grad[1] = ((1 - f[2]) * (v10 - v00) + f[2] * (v11 - v01)) * g.res_inv;
    double gx = (1 - f[2]) * (1 - f[1]) * (v[1][0][0] - v[0][0][0]);
    gx += (1 - f[2]) * f[1] * (v[1][1][0] - v[0][1][0]);
    gx += f[2] * (1 - f[1]) * (v[1][0][1] - v[0][0][1]);
    gx += f[2] * f[1] * (v[1][1][1] - v[0][1][1]);
    grad[0] = gx * g.res_inv;
  }
  return d;
}

// the sample evaluator of the path kernels (path_kernels.hpp): k_h_query_trilinear's arithmetic over the same page-table corners
struct HashPathEval {
  Geom g;
  const int32_t *dir;
  PageTable tab;
  const vox_t *coc;
  __device__ double operator()(const double *p, double *grad) const {
    auto corner = [&](int vx, int vy, int vz) { return h_distance(g, dir, tab, coc, vx - g.gx0, vy - g.gy0, vz - g.gz0); };
    return h_trilinear(g, corner, p, grad);
  }
};
// the page source of the frontier kernel (frontier_kernels.hpp), MAP voxel coordinates: the queries' lookup and GetDistance(Vector3i)
struct HashFrontierPages {
  Geom g;
  const int32_t *dir;
  PageTable tab;
  const vox_t *coc;
  __device__ int64_t addr(int vx, int vy, int vz) const { return h_lookup(g, dir, tab, vx - g.gx0, vy - g.gy0, vz - g.gz0); }
  __device__ double operator()(int vx, int vy, int vz) const { return h_distance(g, dir, tab, coc, vx - g.gx0, vy - g.gy0, vz - g.gz0); }
  // the same value for a caller that already holds the voxel's word (kAct masked): h_distance without its lookup
  __device__ double word_distance(int vx, int vy, int vz, vox_t w) const {
    if (w & kNoCoc) return (double)FIESTA_HIP_INFINITY;
    return sqrt((double)dist2(1, vx, vy, vz, w)) * g.res;
  }
};
// the map side of the reachability flood (reach_kernels.hpp: k_reach_mask), MAP voxel coordinates: 32 voxels from any z are the
// rows of one or two tiles, each found by the queries' map-wide lookup (parked pages answer; no page: all unknown), its observed
// bits gathered from the page's field words; the frontier filter's distance is GetDistance(Vector3i)
struct HashReachSource {
  Geom g;
  const int32_t *dir;
  PageTable tab;
  const vox_t *coc;
  const uint32_t *occbits;
  __device__ void tile_row(int vx, int vy, int vz, uint32_t &o, uint32_t &c) const {  // vz: a multiple of 32
    constexpr int kFar = 1 << 24;  // (pages lie within +-2^24 voxels of the map origin: tile_key)
    o = c = 0u;
    if (vx < -kFar || vx >= kFar || vy < -kFar || vy >= kFar || vz < -kFar || vz >= kFar) return;
    const int64_t a = h_lookup(g, dir, tab, vx - g.gx0, vy - g.gy0, vz - g.gz0);
    if (a < 0) return;
    for (int k = 0; k < 32; ++k) o |= (uint32_t)(coc[a + k] != kUnobserved) << k;
    c = occbits[a >> 5];
  }
  __device__ void row(int vx, int vy, int vz0, uint32_t &o, uint32_t &c) const {
    const int s = vz0 & 31;
    uint32_t o0, c0, o1 = 0, c1 = 0;
    tile_row(vx, vy, vz0 - s, o0, c0);
    if (s) tile_row(vx, vy, vz0 - s + 32, o1, c1);
    o = reach_funnel(o0, o1, s), c = reach_funnel(c0, c1, s);
  }
  __device__ double operator()(int vx, int vy, int vz) const { return h_distance(g, dir, tab, coc, vx - g.gx0, vy - g.gy0, vz - g.gz0); }
};
// the voxel source of the ray query (ray_query_kernels.hpp): the queries' lookup once per TILE -- the page address of the tile the
// ray is in stays in registers (-1: no page, every voxel of it unknown) -- then the voxel's field word and, if it is observed, the
// occupancy word of its row
struct HashRaySource {
  RayGeom g;
  Geom win;  // the window, for the lookup
  const int32_t *dir;
  PageTable tab;
  const vox_t *coc;
  const uint32_t *occbits;
  struct Cache {
    int tx, ty, tz;
    int64_t base, ow;
    uint32_t occ;
  };
  __device__ static Cache fresh() { return Cache{INT32_MIN, 0, 0, -1, -1, 0u}; }
  __device__ int classify(const int *, const int *v, Cache &c) const {
    constexpr int kFar = 1 << 28;  // (pages lie within +-2^24 voxels of the map origin: tile_key)
    if (v[0] < -kFar || v[0] > kFar || v[1] < -kFar || v[1] > kFar || v[2] < -kFar || v[2] > kFar) return FIESTA_HIP_RAY_UNKNOWN;
    const int tx = v[0] >> 4, ty = v[1] >> 4, tz = v[2] >> 5;
    if (tx != c.tx || ty != c.ty || tz != c.tz) {
      c.tx = tx, c.ty = ty, c.tz = tz;
      c.base = h_lookup(win, dir, tab, tx * 16 - win.gx0, ty * 16 - win.gy0, tz * 32 - win.gz0);  // (the tile's first voxel: offset 0 of its page)
    }
    if (c.base < 0) return FIESTA_HIP_RAY_UNKNOWN;
    const int64_t a = c.base + (((v[0] & 15) * 16 + (v[1] & 15)) * 32 + (v[2] & 31));
    if (coc[a] == kUnobserved) return FIESTA_HIP_RAY_UNKNOWN;
    if ((a >> 5) != c.ow) c.ow = a >> 5, c.occ = occbits[a >> 5];
    return ((c.occ >> (a & 31)) & 1u) ? FIESTA_HIP_RAY_OCCUPIED : FIESTA_HIP_RAY_FREE;
  }
};

// A hash-block map as the planner calls see it: the window, the page pool and the map-wide page table (every page answers, resident
// or parked).  The host members are as DenseView's; the map has no outside, so a caller's box is taken as given, clamped to +-2^30.
struct HashView {
  Geom g;
  const int32_t *dir;
  PageTable tab;
  const vox_t *coc;
  const uint32_t *occbits;
  const int32_t *page_gtile;
  int64_t npages;
  int off[3];  // the sources take map voxel coordinates: zero

  HashPathEval path_eval() const { return HashPathEval{g, dir, tab, coc}; }
  HashFrontierPages frontier() const { return HashFrontierPages{g, dir, tab, coc}; }
  const vox_t *field() const { return coc; }  // the skeleton kernel's word source: the page pool, kPageVox words per page
  HashReachSource reach_source() const { return HashReachSource{g, dir, tab, coc, occbits}; }
  HashRaySource ray_source() const { return HashRaySource{ray_geom(g), g, dir, tab, coc, occbits}; }
  // the reach calls' clamped box (lo / hi are not null here), checked before anything is launched; empty: blo[0] > bhi[0]
  void reach_box(const int32_t *lo, const int32_t *hi, int64_t blo[3], int64_t bhi[3]) const {
    bool empty = false;
    for (int k = 0; k < 3; ++k) blo[k] = clamp30(lo[k]), bhi[k] = clamp30(hi[k]), empty = empty || blo[k] > bhi[k];
    if (empty) blo[0] = 1, bhi[0] = 0;
    if (!empty) {  // (each extent is below 2^32)
      const int64_t ex = bhi[0] - blo[0] + 1, ey = bhi[1] - blo[1] + 1, ez = bhi[2] - blo[2] + 1;
      if (ex > kReachMaxVoxels || ey > kReachMaxVoxels || ex * ey > kReachMaxVoxels || ex * ey * ez > kReachMaxVoxels)
        throw Error(FIESTA_HIP_ERR_INVALID, "reach: the box holds more than 2^28 voxels");
    }
  }
  // the corridor calls' window in MAP voxel coordinates: the caller's box clamped to +-2^30, or all of that range; empty: wlo[0] > whi[0]
  void corridor_window(const int32_t *lo, const int32_t *hi, int wlo[3], int whi[3]) const {
    bool any = true;
    for (int c = 0; c < 3; ++c) {
      wlo[c] = lo ? clamp30(lo[c]) : clamp30(INT32_MIN), whi[c] = hi ? clamp30(hi[c]) : clamp30(INT32_MAX);
      any = any && wlo[c] <= whi[c];
    }
    if (!any) wlo[0] = 1, whi[0] = 0;
  }
};

}  // namespace fiesta
