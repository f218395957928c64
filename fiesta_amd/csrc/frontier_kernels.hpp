// fiesta_amd/csrc/frontier_kernels.hpp -- frontier extraction: fiesta_hip_get_frontier_voxels / _dev (include/fiesta_hip.h).
//
// An exploration planner asks after every frame "where does known free space end?": the observed, unoccupied voxels with a
// never-observed 6-neighbour, optionally only those a robot of some radius can stand at.  The map holds everything that answers
// it -- dense maps as two 1-bit-per-voxel maps (observed, occupied), hash-block maps in the field words of their pages -- so the
// query is a bit-parallel stencil over 32-voxel z-words; the distance field is decoded only for the candidates that survive it,
// by the voxel query's own code (the DIST functor: vox_distance on the dense field, h_distance over the page table), so the
// clearance filter sees GetDistance(Vector3i)'s value bit for bit.
//   k_frontier_dense  one lane per z-word (x, y, zw) of the words that intersect the clipped box, lanes along the word index:
//                     obs and occ of the word, obs of the four x / y neighbour words and of the two z-adjacent words (carry bits)
//   k_frontier_hash   one work-group per allocated page (16 x 16 rows of 32 voxels), resident or parked: the rows' observed words are
//                     built by ballot from the page's field words (two rows per wave instruction) into LDS; x / y neighbours
//                     inside the tile are rows of the same page, neighbours across a tile face are read through PAGES::addr,
//                     the map-wide lookup of the queries (no page there: all unknown)
// Both end in frontier_emit: the lanes' candidate counts are prefix-summed across the wave (wave_ops.hpp), ONE integer atomicAdd per
// wave and iteration reserves the wave's range in the output, every lane writes its entries at base + prefix (guarded by the
// capacity).  That atomic is the only one; the SET of (voxel, mask) pairs depends on nothing but the map, the order on scheduling.
#pragma once
#include "../../include/fiesta_hip.h"
#include "common.hpp"
#include "hash_map.hpp"
#include "planner_args.hpp"
#include "wave_ops.hpp"

namespace fiesta {
namespace {  // (planner.hip alone includes this header; the namespace is part of the kernels' symbol names)

struct FrontierBox {  // inclusive; dense maps: local array coordinates, already clipped; hash-block maps: map voxel coordinates
  int x0, y0, z0, x1, y1, z1;
};
struct FrontierOut {
  int32_t *vox;    // 3 per entry, map voxel coordinates (nullable)
  uint8_t *mask;   // u(v) per entry (nullable)
  unsigned long long cap;
  unsigned long long *count;  // the total, whatever the capacity
};

// the bits of a 32-voxel word whose z (z0 = z of bit 0) lies in [lo, hi]
__device__ inline uint32_t frontier_zmask(int z0, int lo, int hi) {
  const int a = max(lo - z0, 0), b = min(hi - z0, 31);
  return a > b ? 0u : ((0xFFFFFFFFu << a) & (0xFFFFFFFFu >> (31 - b)));
}

// cand with the bits removed whose distance is below min_clearance; (x, y, z0): the coordinates DIST takes for bit 0
template <class DIST>
__device__ inline uint32_t frontier_filter(const DIST &dist, uint32_t cand, int x, int y, int z0, double min_clearance) {
  uint32_t keep = cand;
  for (uint32_t b = cand; b; b &= b - 1) {
    const int k = __ffs(b) - 1;
    if (!(dist(x, y, z0 + k) >= min_clearance)) keep &= ~(1u << k);
  }
  return keep;
}

// Appends the set bits of `cand` (voxels (x, y, z0 + bit), map coordinates) with their masks; um .. wp: the word's bits whose
// -x, +x, -y, +y, -z, +z neighbour is unknown.  Every lane of the wave must call it (cand = 0: nothing to add).
__device__ inline void frontier_emit(const FrontierOut &out, uint32_t cand, int x, int y, int z0, uint32_t um, uint32_t up, uint32_t vm,
                                     uint32_t vp, uint32_t wm, uint32_t wp) {
  const int lane = threadIdx.x & 63;
  const int cnt = __popc(cand);
  const int incl = wave_inclusive_sum(cnt);
  const int total = __shfl(incl, 63);
  if (!total) return;  // (uniform across the wave)
  unsigned long long base = 0;
  if (lane == 0) base = atomicAdd(out.count, (unsigned long long)total);
  base = __shfl(base, 0);
  unsigned long long k = base + (unsigned long long)(incl - cnt);
  for (uint32_t b = cand; b; b &= b - 1, ++k) {
    if (k >= out.cap) break;
    const int i = __ffs(b) - 1;
    if (out.vox) out.vox[3 * k] = x, out.vox[3 * k + 1] = y, out.vox[3 * k + 2] = z0 + i;
    if (out.mask)
      out.mask[k] = (uint8_t)(((um >> i) & 1u) | (((up >> i) & 1u) << 1) | (((vm >> i) & 1u) << 2) | (((vp >> i) & 1u) << 3) |
                              (((wm >> i) & 1u) << 4) | (((wp >> i) & 1u) << 5));
  }
}

// DIST: double operator()(int x, int y, int z), local array coordinates -- GetDistance(Vector3i) of that voxel
template <class DIST>
__global__ __launch_bounds__(256) void k_frontier_dense(Geom g, const uint32_t *obsbits, const uint32_t *occbits, FrontierBox b, DIST dist,
                                                        double min_clearance, FrontierOut out) {
  const int zw0 = b.z0 >> 5, nzw = (b.z1 >> 5) - zw0 + 1, ey = b.y1 - b.y0 + 1;
  const int64_t n = (int64_t)(b.x1 - b.x0 + 1) * ey * nzw;
  // (the trip count is the same for every lane of the work-group: frontier_emit needs whole waves)
  for (int64_t base = blockIdx.x * (int64_t)blockDim.x; base < n; base += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = base + threadIdx.x;
    uint32_t cand = 0, um = 0, up = 0, vm = 0, vp = 0, wm = 0, wp = 0;
    int x = 0, y = 0, zw = 0;
    if (i < n) {
      zw = zw0 + (int)(i % nzw), y = b.y0 + (int)((i / nzw) % ey), x = b.x0 + (int)(i / ((int64_t)nzw * ey));
      const int64_t wi = ((int64_t)x * g.ny + y) * g.nzw + zw;
      const uint32_t obs = obsbits[wi];
      // the padding bits of the last word are zero in the bitmap; they are no voxels (not free) and, as +z neighbours, outside
      const uint32_t valid = (zw == g.nzw - 1 && (g.nz & 31)) ? ((1u << (g.nz & 31)) - 1u) : 0xFFFFFFFFu;
      const uint32_t fre = obs & ~occbits[wi] & valid & frontier_zmask(zw * 32, b.z0, b.z1);
      if (fre) {
        // a neighbour outside the array is not unknown
        if (x > 0) um = ~obsbits[wi - (int64_t)g.ny * g.nzw] & fre;
        if (x < g.nx - 1) up = ~obsbits[wi + (int64_t)g.ny * g.nzw] & fre;
        if (y > 0) vm = ~obsbits[wi - g.nzw] & fre;
        if (y < g.ny - 1) vp = ~obsbits[wi + g.nzw] & fre;
        const uint32_t ext = obs | ~valid;
        const uint32_t below = zw > 0 ? (obsbits[wi - 1] >> 31) : 1u;
        const uint32_t above = zw < g.nzw - 1 ? (obsbits[wi + 1] & 1u) : 1u;
        wm = ~((ext << 1) | below) & fre;
        wp = ~((ext >> 1) | (above << 31)) & fre;
        cand = um | up | vm | vp | wm | wp;
        if (cand && min_clearance > 0) cand = frontier_filter(dist, cand, x, y, zw * 32, min_clearance);
      }
    }
    frontier_emit(out, cand, x + g.gx0, y + g.gy0, zw * 32 + g.gz0, um, up, vm, vp, wm, wp);
  }
}

// PAGES: int64_t addr(int vx, int vy, int vz) -- pool address of MAP voxel (vx, vy, vz), -1: no page holds it -- and
//        double operator()(int vx, int vy, int vz) -- GetDistance(Vector3i) of that voxel.
// One work-group of 256 lanes per page; lane = row = (x & 15) * 16 + (y & 15).
template <class PAGES>
__device__ inline uint32_t frontier_row_obs(const PAGES &pg, const vox_t *coc, int vx, int vy, int vz0) {
  const int64_t a = pg.addr(vx, vy, vz0);  // (vz0 is a multiple of 32: the row is 32 consecutive words)
  if (a < 0) return 0u;
  uint32_t m = 0;
  for (int k = 0; k < 32; ++k) m |= (uint32_t)(coc[a + k] != kUnobserved) << k;
  return m;
}
template <class PAGES>
__global__ __launch_bounds__(256) void k_frontier_hash(const int32_t *page_gtile, int64_t npages, const vox_t *coc, const uint32_t *occbits,
                                                       FrontierBox b, PAGES pg, double min_clearance, FrontierOut out) {
  __shared__ uint32_t s_obs[HashMap::kPageRows];
  const int row = threadIdx.x, lane = row & 63, wave = row >> 6, lx = row >> 4, ly = row & 15;
  for (int64_t page = blockIdx.x; page < npages; page += gridDim.x) {
    const int X0 = page_gtile[3 * page] * 16, Y0 = page_gtile[3 * page + 1] * 16, Z0 = page_gtile[3 * page + 2] * 32;
    if (X0 > b.x1 || X0 + 15 < b.x0 || Y0 > b.y1 || Y0 + 15 < b.y0 || Z0 > b.z1 || Z0 + 31 < b.z0) continue;  // (uniform)
    const vox_t *pc = coc + page * HashMap::kPageVox;
    for (int i = 0; i < 32; ++i) {  // rows wave * 64 + 2 i and + 2 i + 1: 64 consecutive field words
      const unsigned long long m = __ballot(pc[(wave * 64 + 2 * i) * 32 + lane] != kUnobserved);
      if (lane == 0) s_obs[wave * 64 + 2 * i] = (uint32_t)m, s_obs[wave * 64 + 2 * i + 1] = (uint32_t)(m >> 32);
    }
    __syncthreads();
    const int x = X0 + lx, y = Y0 + ly;
    uint32_t cand = 0, um = 0, up = 0, vm = 0, vp = 0, wm = 0, wp = 0;
    const uint32_t obs = s_obs[row];
    uint32_t fre = 0;
    if (x >= b.x0 && x <= b.x1 && y >= b.y0 && y <= b.y1) fre = obs & ~occbits[page * HashMap::kPageRows + row] & frontier_zmask(Z0, b.z0, b.z1);
    if (fre) {
      um = ~(lx > 0 ? s_obs[row - 16] : frontier_row_obs(pg, coc, x - 1, y, Z0)) & fre;
      up = ~(lx < 15 ? s_obs[row + 16] : frontier_row_obs(pg, coc, x + 1, y, Z0)) & fre;
      vm = ~(ly > 0 ? s_obs[row - 1] : frontier_row_obs(pg, coc, x, y - 1, Z0)) & fre;
      vp = ~(ly < 15 ? s_obs[row + 1] : frontier_row_obs(pg, coc, x, y + 1, Z0)) & fre;
      uint32_t below = 0, above = 0;  // only bit 0 / bit 31 of the word ask for them
      if (fre & 1u) {
        const int64_t a = pg.addr(x, y, Z0 - 1);
        below = a >= 0 && coc[a] != kUnobserved;
      }
      if (fre >> 31) {
        const int64_t a = pg.addr(x, y, Z0 + 32);
        above = a >= 0 && coc[a] != kUnobserved;
      }
      wm = ~((obs << 1) | below) & fre;
      wp = ~((obs >> 1) | (above << 31)) & fre;
      cand = um | up | vm | vp | wm | wp;
      if (cand && min_clearance > 0) cand = frontier_filter(pg, cand, x, y, Z0, min_clearance);
    }
    frontier_emit(out, cand, x, y, Z0, um, up, vm, vp, wm, wp);
    __syncthreads();  // (the next page overwrites s_obs)
  }
}

}  // namespace
}  // namespace fiesta
