// fiesta_amd/csrc/skeleton_kernels.hpp -- skeleton voxels: fiesta_hip_get_skeleton_voxels / _dev (include/fiesta_hip.h).
//
// Every field word names the voxel's closest obstacle (its SITE).  Where two 6-neighbours name sites that lie apart and the
// bisector plane of the two sites passes between the voxels, the field has a ridge: the generalised Voronoi skeleton of free space,
// the by-product of an incremental ESDF that no other planner call reads.  The rule is written once (skel_neighbour), over sites in MAP
// voxel coordinates, integers only; the two kernels differ in where the seven words of a voxel come from.
//   k_skeleton_dense  a WAVE per row (x, y) under the clipped box, 64-voxel z-chunk after chunk, lanes along z: the chunk's two observed /
//                     occupied bitmap words decide first whether the chunk holds a free voxel in the box at all (if not, the field is
//                     not touched); then one coalesced load of the chunk's own words, the z neighbours from the adjacent lanes by
//                     shuffle (lanes 0 / 63: one load each), the four x / y neighbours as coalesced loads of the adjacent rows
//   k_skeleton_hash   one work-group per allocated page, resident or parked: the page's 8192 field words staged in LDS (32 KiB);
//                     neighbours inside the tile are LDS reads, neighbours across a tile face go through PAGES::addr, the map-wide
//                     lookup of the queries (no page there: no site)
// Both end in the frontier call's compaction, generalised to waves that nearly all hold survivors (a sixth of a map's free voxels
// lie on a ridge): a wave first collects its rows in LDS (SkelBuf: the survivors' prefix over the wave is a ballot and a
// popcount, the flags being single bits) and reserves their place in the output when the buffer could not take 64 more, and once
// at its end: ONE integer atomicAdd per wave and such iteration, every lane then writes rows at base + index (guarded by the
// capacity).  That atomic is the only one; the SET of rows depends on nothing but the map.  (One atomicAdd per 64 voxels, the
// frontier kernel's form, was measured first: all of them hit one counter, which serves some 70 million a second -- 25 ms for the
// two million chunks of a 512^3 map, 150 times one pass over its field.)
#pragma once
#include "../../include/fiesta_hip.h"
#include "common.hpp"
#include "dense_read.hpp"
#include "frontier_kernels.hpp"
#include "hash_map.hpp"
#include "planner_args.hpp"
#include "wave_ops.hpp"

namespace fiesta {
namespace {  // (planner.hip alone includes this header; the namespace is part of the kernels' symbol names)

struct SkeletonOut {
  int32_t *vox;   // 3 per entry, map voxel coordinates (nullable)
  uint8_t *mask;  // r(v) per entry (nullable)
  int32_t *d2;    // the voxel's own squared distance (nullable)
  int32_t *sep2;  // the largest site separation over the set bits of r(v) (nullable)
  unsigned long long cap;
  unsigned long long *count;  // the total, whatever the capacity
};

// a voxel in map voxel coordinates, or a voxel MINUS a site
struct SkelPt {
  int x, y, z;
};
// v minus the site of field word w held by MAP voxel v; the caller has tested !(w & kNoCoc)
__device__ inline SkelPt skel_offset(int wrap, const SkelPt &v, vox_t w) {
  SkelPt o;
  coc_offset(wrap, v.x, v.y, v.z, w, o.x, o.y, o.z);
  return o;
}
// One neighbour's verdict, ridge(v, n).  A = v - a (a: v's site), d2v = |A|^2; k: the neighbour's bit in the mask's order, n = v + e;
// nw: its word with kAct masked, or kUnobserved where the neighbour is outside the array, has no page or is not observed.
// With b the neighbour's site and B = v - b:  sep2 = |a - b|^2 = |B - A|^2,  g(v) = |v - b|^2 - |v - a|^2 = |B|^2 - d2v,  and, g being
// linear,  g(n) = g(v) + 2 e . (a - b).  ridge iff a and b lie at least sqrt(min_sep2) apart, the bisector plane of a and b passes
// between v and n (g >= 0 on a's side) and v is at least as close to it as n; a pair the field puts on the wrong side (g(v) < 0 or
// g(n) > 0: the field is no exact transform) is skipped.  A ridge sets bit k of r and raises best to its separation.
// Integers only: a site lies within 1774 voxels (sqrt(3) * 1024) of the voxel that names it, so every coordinate difference below
// is at most 2 * 1774 + 1 in magnitude and every sum of three squares below 2^26 (d2 and sep2 themselves below 2^22): int32.
__device__ inline void skel_neighbour(int wrap, const SkelPt &v, const SkelPt &A, int32_t d2v, int k, vox_t nw, int32_t min_sep2, uint32_t &r,
                                      int32_t &best) {
  if (nw & kNoCoc) return;  // (never observed, or observed without an obstacle: no site, whatever link the word keeps)
  const int ex = (k == 1) - (k == 0), ey = (k == 3) - (k == 2), ez = (k == 5) - (k == 4);
  SkelPt B = skel_offset(wrap, SkelPt{v.x + ex, v.y + ey, v.z + ez}, nw);  // n - b
  B.x -= ex, B.y -= ey, B.z -= ez;                                        // v - b
  const int dx = B.x - A.x, dy = B.y - A.y, dz = B.z - A.z;               // a - b
  const int32_t sep2 = dx * dx + dy * dy + dz * dz;
  const int32_t gv = B.x * B.x + B.y * B.y + B.z * B.z - d2v, gn = gv + 2 * (ex * dx + ey * dy + ez * dz);
  if (sep2 >= min_sep2 && gv >= 0 && gn <= 0 && gv <= -gn) r |= 1u << k, best = max(best, sep2);
}

// One wave's collected rows, in LDS as a structure of arrays.  d2 and sep2 are below 2^22 (skel_neighbour), so the mask rides on d2.
template <int ROWS>
struct SkelBuf {
  int32_t x[ROWS], y[ROWS], z[ROWS];
  uint32_t d2r[ROWS];  // d2 | r(v) << 24
  int32_t sep2[ROWS];
};
// Moves the wave's n collected rows to the output.  Every lane of the wave must call it; n is the same in all of them.
template <int ROWS>
__device__ inline void skeleton_flush(const SkeletonOut &out, const SkelBuf<ROWS> &buf, int &n) {
  if (n) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (the rows are another lane's writes)
    const int lane = threadIdx.x & 63;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(out.count, (unsigned long long)n);
    base = __shfl(base, 0);
    for (int j = lane; j < n; j += 64) {
      const unsigned long long k = base + (unsigned long long)j;
      if (k >= out.cap) break;
      if (out.vox) out.vox[3 * k] = buf.x[j], out.vox[3 * k + 1] = buf.y[j], out.vox[3 * k + 2] = buf.z[j];
      if (out.mask) out.mask[k] = (uint8_t)(buf.d2r[j] >> 24);
      if (out.d2) out.d2[k] = (int32_t)(buf.d2r[j] & 0xFFFFFFu);
      if (out.sep2) out.sep2[k] = buf.sep2[j];
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (the next rows overwrite these)
  }
  n = 0;
}
// Collects this lane's row if `keep`, after making room for a whole wave's.  Every lane of the wave must call it.
template <int ROWS>
__device__ inline void skeleton_collect(const SkeletonOut &out, SkelBuf<ROWS> &buf, int &n, bool keep, const SkelPt &v, uint32_t r, int32_t d2,
                                        int32_t sep2) {
  if (n > ROWS - 64) skeleton_flush(out, buf, n);  // (uniform across the wave)
  const unsigned long long m = __ballot(keep);
  if (keep) {
    const int j = n + __popcll(m & ((1ull << (threadIdx.x & 63)) - 1ull));
    buf.x[j] = v.x, buf.y[j] = v.y, buf.z[j] = v.z, buf.d2r[j] = (uint32_t)d2 | (r << 24), buf.sep2[j] = sep2;
  }
  n += __popcll(m);
}
constexpr int kSkelDenseRows = 512, kSkelHashRows = 256;  // rows a wave collects per atomicAdd: 10 KiB / 5 KiB of LDS per wave

// b: the caller's box clipped to the array, local array coordinates.  A work-group is four independent waves.  The clearance filter
// is GetDistance(Vector3i) of the word already in the lane's register: word_distance (dense_read.hpp), the voxel query's arithmetic.
__global__ __launch_bounds__(256) void k_skeleton_dense(Geom g, const vox_t *coc, const uint32_t *obsbits, const uint32_t *occbits,
                                                        FrontierBox b, int32_t min_sep2, double min_clearance, SkeletonOut out) {
  __shared__ SkelBuf<kSkelDenseRows> s_rows[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  SkelBuf<kSkelDenseRows> &rows = s_rows[wave];
  int n_rows = 0;
  const int c0 = b.z0 >> 6, c1 = b.z1 >> 6;
  const uint32_t ey = b.y1 - b.y0 + 1, n = (uint32_t)(b.x1 - b.x0 + 1) * ey;  // rows (x, y) of the box: fewer than 2^31
  // A wave takes whole rows, chunk after chunk (consecutive waves: consecutive y).  The chunk is the same for every lane of a wave:
  // the shuffles and skeleton_collect see whole waves.
  for (uint32_t i = blockIdx.x * 4u + wave; i < n; i += gridDim.x * 4u) {
    const int y = b.y0 + (int)(i % ey), x = b.x0 + (int)(i / ey);
    for (int c = c0; c <= c1; ++c) {
      const int z = c * 64 + lane, zw = z >> 5;  // (lanes 0..31: bitmap word 2c, lanes 32..63: word 2c + 1)
      bool fre = false;
      if (zw < g.nzw) {
        const int64_t wi = ((int64_t)x * g.ny + y) * g.nzw + zw;
        fre = ((obsbits[wi] & ~occbits[wi]) >> (z & 31)) & 1u;  // (the padding bits of a row's last word are zero)
      }
      fre = fre && z < g.nz && z >= b.z0 && z <= b.z1;
      if (!__ballot(fre)) continue;  // no free voxel of the box in these 64: the field is not read
      const bool in = z < g.nz;
      const int64_t vi = g.idx(x, y, in ? z : 0);
      const vox_t w = in ? (coc[vi] & ~kAct) : kUnobserved;
      vox_t nb[6];
      nb[4] = __shfl_up(w, 1, 64), nb[5] = __shfl_down(w, 1, 64);
      if (lane == 0) nb[4] = (in && z > 0) ? (coc[vi - 1] & ~kAct) : kUnobserved;
      if (lane == 63) nb[5] = (z + 1 < g.nz) ? (coc[vi + 1] & ~kAct) : kUnobserved;
      bool keep = false;
      uint32_t r = 0;
      int32_t sep2 = 0, d2 = 0;
      const SkelPt v{x + g.gx0, y + g.gy0, z + g.gz0};
      if (fre && !(w & kNoCoc)) {
        const int64_t sx = (int64_t)g.ny * g.nz;
        nb[0] = x > 0 ? (coc[vi - sx] & ~kAct) : kUnobserved;
        nb[1] = x < g.nx - 1 ? (coc[vi + sx] & ~kAct) : kUnobserved;
        nb[2] = y > 0 ? (coc[vi - g.nz] & ~kAct) : kUnobserved;
        nb[3] = y < g.ny - 1 ? (coc[vi + g.nz] & ~kAct) : kUnobserved;
        const SkelPt A = skel_offset(g.wrap, v, w);
        d2 = A.x * A.x + A.y * A.y + A.z * A.z;  // (dist2 of common.hpp)
#pragma unroll
        for (int k = 0; k < 6; ++k) skel_neighbour(g.wrap, v, A, d2, k, nb[k], min_sep2, r, sep2);
        keep = r != 0;
        if (keep && min_clearance > 0) keep = word_distance(g, w, x, y, z) >= min_clearance;
      }
      skeleton_collect(out, rows, n_rows, keep, v, r, d2, sep2);
    }
  }
  skeleton_flush(out, rows, n_rows);
}

// PAGES: int64_t addr(int vx, int vy, int vz) as k_frontier_hash's, and double word_distance(int vx, int vy, int vz, vox_t w) --
// GetDistance(Vector3i) of MAP voxel (vx, vy, vz) whose word (kAct masked) is w.  b: map voxel coordinates.  One work-group of 256
// lanes per page; in trip i lane t holds the page's word i * 256 + t: row (x & 15) * 16 + (y & 15) = i * 8 + (t >> 5), z & 31 = t & 31.
template <class PAGES>
__global__ __launch_bounds__(256) void k_skeleton_hash(const int32_t *page_gtile, int64_t npages, const vox_t *coc, const uint32_t *occbits,
                                                       FrontierBox b, PAGES pg, int32_t min_sep2, double min_clearance, SkeletonOut out) {
  __shared__ vox_t s_w[HashMap::kPageVox];
  __shared__ SkelBuf<kSkelHashRows> s_rows[4];
  SkelBuf<kSkelHashRows> &rows = s_rows[threadIdx.x >> 6];
  int n_rows = 0;
  const int t = threadIdx.x;
  for (int64_t page = blockIdx.x; page < npages; page += gridDim.x) {
    const int X0 = page_gtile[3 * page] * 16, Y0 = page_gtile[3 * page + 1] * 16, Z0 = page_gtile[3 * page + 2] * 32;
    if (X0 > b.x1 || X0 + 15 < b.x0 || Y0 > b.y1 || Y0 + 15 < b.y0 || Z0 > b.z1 || Z0 + 31 < b.z0) continue;  // (uniform)
    const vox_t *pc = coc + page * HashMap::kPageVox;
    for (int i = 0; i < HashMap::kPageVox / 256; ++i) s_w[i * 256 + t] = pc[i * 256 + t] & ~kAct;  // (unobserved keeps bit 31)
    __syncthreads();
    // a neighbour's word: inside the tile from LDS, else through the map-wide lookup
    auto word = [&](int lx, int ly, int lz) -> vox_t {
      if ((unsigned)lx < 16u && (unsigned)ly < 16u && (unsigned)lz < 32u) return s_w[(lx * 16 + ly) * 32 + lz];
      const int64_t a = pg.addr(X0 + lx, Y0 + ly, Z0 + lz);
      return a < 0 ? kUnobserved : (coc[a] & ~kAct);
    };
    for (int i = 0; i < HashMap::kPageVox / 256; ++i) {  // (the same trip count for every lane: skeleton_collect needs whole waves)
      const int o = i * 256 + t, row = o >> 5, lx = row >> 4, ly = row & 15, lz = o & 31;
      const SkelPt v{X0 + lx, Y0 + ly, Z0 + lz};
      const vox_t w = s_w[o];
      bool keep = false;
      uint32_t r = 0;
      int32_t sep2 = 0, d2 = 0;
      if (!(w & kNoCoc) && !((occbits[page * HashMap::kPageRows + row] >> lz) & 1u) && v.x >= b.x0 && v.x <= b.x1 && v.y >= b.y0 &&
          v.y <= b.y1 && v.z >= b.z0 && v.z <= b.z1) {
        const SkelPt A = skel_offset(1, v, w);
        d2 = A.x * A.x + A.y * A.y + A.z * A.z;  // (dist2 of common.hpp)
#pragma unroll 1  // (one copy of the lookup, not six: the page table's search is long and the kernel's scalar registers are few)
        for (int k = 0; k < 6; ++k)
          skel_neighbour(1, v, A, d2, k, word(lx + (k == 1) - (k == 0), ly + (k == 3) - (k == 2), lz + (k == 5) - (k == 4)), min_sep2, r, sep2);
        keep = r != 0;
        if (keep && min_clearance > 0) keep = pg.word_distance(v.x, v.y, v.z, w) >= min_clearance;
      }
      skeleton_collect(out, rows, n_rows, keep, v, r, d2, sep2);
    }
    __syncthreads();  // (the next page overwrites s_w)
  }
  skeleton_flush(out, rows, n_rows);
}

}  // namespace
}  // namespace fiesta
