// fiesta_amd/csrc/corridor_kernels.hpp -- free-space corridors: fiesta_hip_free_boxes / _dev and fiesta_hip_path_corridor / _dev
// (include/fiesta_hip.h).
//
// A trajectory optimiser takes a safe flight corridor, a short sequence of overlapping axis-aligned boxes of traversable space
// around a path, not a voxel staircase.  Both calls rest on one device routine run by ONE WAVE of 64:
//   corridor_inflate<SRC>    grows a box face by face (-x, +x, -y, +y, -z, +z in turn) while the slab beyond the face is traversable
//                            and inside the window W.  The box, the growth counts and the stop codes are wave-uniform; a slab test
//                            spreads the slab's items over the lanes and decides with a ballot.  For the x and y faces an item is one
//                            word of traversability bits of a z-row of the slab (corridor_word: SRC::row at any z, masked to the
//                            box's z-range, so an unaligned z origin and a short last word cost nothing extra); for the z faces an
//                            item is one (x, y) column, a word of a single bit.
//   k_free_boxes<SRC>        a wave per seed, grid-stride
//   k_corridor_count<SRC>    a wave per path: checks the path, walks the voxel chain of every segment (candidate A, then B), runs the
//                            greedy and writes the per-path outputs and the number of boxes into offsets[p + 1]
//   k_reach_path_scan        (reach_path_kernels.hpp, as it is) offsets -> running totals
//   k_corridor_write<SRC>    the greedy again, storing box k of path p at offsets[p] + k if that index lies below the capacity
// A segment's chain: the reference traversal (ray_walk.hpp: dda_walk, f64) is computed redundantly by every lane; lane k & 63 keeps
// voxel k, and every 64 voxels the lanes test theirs and a ballot finds the first that is not traversable.  The axis of every
// step is RECORDED, two bits per step, in two 64-bit registers per lane (lane l: steps 64 l .. 64 l + 63; a chain has at most 4095
// steps), so the visit replays the chain from the record with a shuffle per step -- forwards for A, backwards for B, which is the
// reverse of the traversal from the far end -- and the f64 traversal runs once per candidate.
// All arithmetic is integer apart from the traversal, the clearance comparison and the metric corners, and every decision is
// wave-uniform and follows the sequential rule of the header: the outputs do not depend on the grid or the scheduling.  No atomics,
// no LDS, no waiting of one work-group for another; every loop is bounded (6 * (max_grow + 1) face tests per box, 8192 iterations
// and 4096 voxels per traversal).
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>

#include "../../include/fiesta_hip.h"
#include "common.hpp"
#include "planner.hpp"
#include "planner_args.hpp"
#include "frontier_kernels.hpp"
#include "ray_walk.hpp"
#include "reach_kernels.hpp"
#include "reach_path_kernels.hpp"

namespace fiesta {
namespace {  // (planner.hip alone includes this header; the namespace is part of the kernels' symbol names)

constexpr int kCorridorBlock = 256, kCorridorMaxBlocks = 4096;
constexpr int kCorridorCoordMax = 1 << 30;
constexpr int kCorridorManhattan = 4095;

// W in MAP voxel coordinates (inclusive; lo[0] > hi[0]: empty), and what SRC's coordinates are behind the map's
struct CorridorWin {
  int lo[3], hi[3];
  int off[3];
  double res, org[3];
};
struct CorridorRule {
  double min_clearance;
  int through_unknown, max_grow;
};
struct FreeBoxOut {  // device pointers, each nullable
  int32_t *box;
  double *box_pos;
  uint8_t *stop;
  int64_t *volume;
  int32_t *status;
};
struct CorridorOut {  // device pointers; offsets is never null
  int64_t *offsets;
  int32_t *boxes;
  double *boxes_pos;
  uint8_t *stop;
  int32_t *entry;
  int32_t *status, *n_chain, *blocked_segment, *blocked_vox;
  int64_t capacity;
};
struct CorridorIn {  // the waypoints and their CSR offsets
  const int32_t *wp;
  int64_t n_wp;
  const int64_t *poff;
  int64_t n;
};
struct CorridorBox {  // wave-uniform; named fields, never indexed
  int lx, ly, lz, hx, hy, hz;
  unsigned stop;  // four bits per face
  __device__ int stop_of(int f) const { return (int)((stop >> (4 * f)) & 15u); }
  __device__ bool holds(int x, int y, int z) const { return x >= lx && x <= hx && y >= ly && y <= hy && z >= lz && z <= hz; }
  __device__ int64_t volume() const { return ((int64_t)hx - lx + 1) * ((int64_t)hy - ly + 1) * ((int64_t)hz - lz + 1); }
};

// A copy of a kernel argument whose words the compiler must take for lane-dependent, so that it keeps them in vector registers: the
// arguments of these kernels (the source's geometry and pointers, the window, the outputs) are some 90 scalar registers that would
// otherwise stay live through every loop and be spilled.  Each word is OR-ed with a zero that only the hardware knows to be zero.
template <class T>
__device__ inline T corridor_in_vgprs(const T &t) {
  static_assert(sizeof(T) % 4 == 0, "whole words");
  uint32_t zero;
  asm volatile("v_mov_b32 %0, 0" : "=v"(zero));
  uint32_t words[sizeof(T) / 4];
  __builtin_memcpy(words, &t, sizeof(T));
#pragma unroll
  for (size_t i = 0; i < sizeof(T) / 4; ++i) words[i] |= zero;
  T out;
  __builtin_memcpy(&out, words, sizeof(T));
  return out;
}

__device__ __forceinline__ bool corridor_in_win(const CorridorWin &w, int x, int y, int z) {
  return x >= w.lo[0] && x <= w.hi[0] && y >= w.lo[1] && y <= w.hi[1] && z >= w.lo[2] && z <= w.hi[2];
}

// traversability bits of the nv <= 32 voxels (x, y, z0 + k) -- MAP coordinates, all inside W: k_reach_mask's word
template <class SRC>
__device__ __forceinline__ uint32_t corridor_word(const SRC &src, const CorridorWin &w, const CorridorRule &r, int x, int y, int z0, int nv) {
  const uint32_t valid = nv == 32 ? 0xFFFFFFFFu : ((1u << nv) - 1u);
  const int sx = x - w.off[0], sy = y - w.off[1], sz = z0 - w.off[2];
  uint32_t obs, occ;
  src.row(sx, sy, sz, obs, occ);
  uint32_t fre = obs & ~occ & valid;
  if (fre && r.min_clearance > 0) fre = frontier_filter(src, fre, sx, sy, sz, r.min_clearance);
  return (fre | (r.through_unknown ? (~obs & valid) : 0u)) ^ valid;  // the bits that are NOT traversable
}
template <class SRC>
__device__ __forceinline__ bool corridor_voxel(const SRC &src, const CorridorWin &w, const CorridorRule &r, int x, int y, int z) {
  return corridor_in_win(w, x, y, z) && corridor_word(src, w, r, x, y, z, 1) == 0u;
}

// The slab with coordinate c on axis a over the box's other two axes, all of it inside W: wave-uniform result.  Items are spread
// over the lanes: for the x and y faces (row along the other horizontal axis, z-word), for the z faces one (x, y) column each.
template <class SRC>
__device__ __forceinline__ bool corridor_slab(const SRC &src, const CorridorWin &w, const CorridorRule &r, const CorridorBox &b, int a, int c) {
  const int lane = threadIdx.x & 63;
  const int ez = a == 2 ? 1 : b.hz - b.lz + 1, nzw = (ez + 31) >> 5;  // (a z face: one word of one bit per column)
  const int ey = b.hy - b.ly + 1;
  const int rows = a == 0 ? ey : (a == 1 ? b.hx - b.lx + 1 : (b.hx - b.lx + 1) * ey);
  const int n = rows * nzw, z0 = a == 2 ? c : b.lz;
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    bool ok = true;
    if (i < n) {
      const int zw = i % nzw, row = i / nzw, nv = min(32, ez - 32 * zw);
      const int x = a == 0 ? c : (a == 1 ? b.lx + row : b.lx + row / ey), y = a == 0 ? b.ly + row : (a == 1 ? c : b.ly + row % ey);
      ok = corridor_word(src, w, r, x, y, z0 + 32 * zw, nv) == 0u;
    }
    if (__ballot(!ok)) return false;
  }
  return true;
}

// inflate(lo0, hi0, max_grow) of the header; b holds the seed box on entry (every voxel of it traversable and inside W)
template <class SRC>
__device__ __forceinline__ void corridor_inflate(const SRC &src, const CorridorWin &w, const CorridorRule &r, CorridorBox &b) {
  unsigned long long g = 0ull;  // ten bits per face
  int open = 6;
  unsigned stop = 0u;
  // the box and the window in scalars of their own, chosen by VALUE: a choice between fields of a struct would be an indexed access
  int lx = b.lx, ly = b.ly, lz = b.lz, hx = b.hx, hy = b.hy, hz = b.hz;
  const int wl0 = w.lo[0], wl1 = w.lo[1], wl2 = w.lo[2], wh0 = w.hi[0], wh1 = w.hi[1], wh2 = w.hi[2];
  while (open > 0) {  // (every face test grows or stops a face: at most 6 * (max_grow + 1) of them)
    for (int f = 0; f < 6; ++f) {
      if ((stop >> (4 * f)) & 15u) continue;
      const int a = f >> 1, gf = (int)((g >> (10 * f)) & 1023ull);
      const int lo_a = a == 0 ? lx : (a == 1 ? ly : lz), hi_a = a == 0 ? hx : (a == 1 ? hy : hz);
      const int wlo = a == 0 ? wl0 : (a == 1 ? wl1 : wl2), whi = a == 0 ? wh0 : (a == 1 ? wh1 : wh2);
      const int c = (f & 1) ? hi_a + 1 : lo_a - 1;
      int code = 0;
      if (gf == r.max_grow)
        code = FIESTA_HIP_CORRIDOR_STOP_LIMIT;
      else if (c < wlo || c > whi)
        code = FIESTA_HIP_CORRIDOR_STOP_EDGE;
      else if (!corridor_slab(src, w, r, CorridorBox{lx, ly, lz, hx, hy, hz, 0u}, a, c))
        code = FIESTA_HIP_CORRIDOR_STOP_BLOCKED;
      if (code) {
        stop |= (unsigned)code << (4 * f);
        --open;
        continue;
      }
      g += 1ull << (10 * f);
      lx = f == 0 ? c : lx, hx = f == 1 ? c : hx, ly = f == 2 ? c : ly, hy = f == 3 ? c : hy, lz = f == 4 ? c : lz, hz = f == 5 ? c : hz;
    }
  }
  b = CorridorBox{lx, ly, lz, hx, hy, hz, stop};
}

// lane 0 stores a box: `box` 6 i32, `stop` 6 u8, `pos` 6 f64 (each nullable)
__device__ __forceinline__ void corridor_store(const CorridorWin &w, const CorridorBox &b, int32_t *box, uint8_t *stop, double *pos) {
  if (box) box[0] = b.lx, box[1] = b.ly, box[2] = b.lz, box[3] = b.hx, box[4] = b.hy, box[5] = b.hz;
  if (stop)
    for (int f = 0; f < 6; ++f) stop[f] = (uint8_t)b.stop_of(f);
  if (pos) {
    pos[0] = (double)b.lx * w.res + w.org[0], pos[1] = (double)b.ly * w.res + w.org[1], pos[2] = (double)b.lz * w.res + w.org[2];
    pos[3] = ((double)b.hx + 1.0) * w.res + w.org[0], pos[4] = ((double)b.hy + 1.0) * w.res + w.org[1];
    pos[5] = ((double)b.hz + 1.0) * w.res + w.org[2];
  }
}

template <class SRC>
__global__ __launch_bounds__(kCorridorBlock) void k_free_boxes(SRC src_, CorridorWin w_, CorridorRule r_, const int32_t *seeds, int64_t n, FreeBoxOut o_) {
  const SRC src = corridor_in_vgprs(src_);
  const CorridorWin w = corridor_in_vgprs(w_);
  const CorridorRule r = corridor_in_vgprs(r_);
  const FreeBoxOut o = corridor_in_vgprs(o_);
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * (kCorridorBlock / 64);
  for (int64_t i = blockIdx.x * (int64_t)(kCorridorBlock / 64) + (threadIdx.x >> 6); i < n; i += stride) {
    const int x = seeds[3 * i], y = seeds[3 * i + 1], z = seeds[3 * i + 2];
    CorridorBox b{x, y, z, x, y, z, 0u};
    int st = FIESTA_HIP_FREE_BOX_OK;
    if (!corridor_in_win(w, x, y, z))
      st = FIESTA_HIP_FREE_BOX_OUTSIDE;
    else if (corridor_word(src, w, r, x, y, z, 1) != 0u)
      st = FIESTA_HIP_FREE_BOX_BLOCKED;
    if (st == FIESTA_HIP_FREE_BOX_OK)
      corridor_inflate(src, w, r, b);
    else
      b = CorridorBox{INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN, 0u};
    if (lane != 0) continue;
    if (o.status) o.status[i] = st;
    if (o.volume) o.volume[i] = st ? 0 : b.volume();
    corridor_store(w, b, o.box ? o.box + 6 * i : nullptr, o.stop ? o.stop + 6 * i : nullptr, st || !o.box_pos ? nullptr : o.box_pos + 6 * i);
    if (st && o.box_pos)
      for (int c = 0; c < 6; ++c) o.box_pos[6 * i + c] = __longlong_as_double(0x7FF8000000000000ll);
  }
}

// ---- path corridors --------------------------------------------------------------------------------------------------------

// The greedy's state, wave-uniform.
struct CorridorWalk {
  CorridorBox last;
  int nboxes;          // boxes so far
  int idx;             // chain voxels visited
  int px, py, pz;      // prev (valid if idx > 0)
};

template <class SRC, bool WRITE>
__device__ __forceinline__ void corridor_visit(const SRC &src, const CorridorWin &w, const CorridorRule &r, const CorridorOut &o, int64_t first, CorridorWalk &s,
                                      int x, int y, int z) {
  if (!(s.nboxes > 0 && s.last.holds(x, y, z))) {
    const bool fresh = s.idx == 0;
    s.last = CorridorBox{fresh ? x : min(s.px, x), fresh ? y : min(s.py, y), fresh ? z : min(s.pz, z),
                         fresh ? x : max(s.px, x), fresh ? y : max(s.py, y), fresh ? z : max(s.pz, z), 0u};
    corridor_inflate(src, w, r, s.last);
    const int64_t at = first + s.nboxes;
    if (WRITE && at < o.capacity && (threadIdx.x & 63) == 0) {
      corridor_store(w, s.last, o.boxes ? o.boxes + 6 * at : nullptr, o.stop ? o.stop + 6 * at : nullptr, o.boxes_pos ? o.boxes_pos + 6 * at : nullptr);
      if (o.entry) o.entry[at] = s.idx;
    }
    ++s.nboxes;
  }
  s.px = x, s.py = y, s.pz = z;
  ++s.idx;
}

// The traversal from voxel p to voxel q with every emitted voxel tested, 64 at a time, and every step's axis recorded (rec0 / rec1:
// this lane's 64 steps, two bits each).  count: voxels emitted (on failure: up to the failing batch); (ex, ey, ez): the last one
// emitted.  Returns true if all were traversable; else (fx, fy, fz) is the first that was not.
template <class SRC>
__device__ __forceinline__ bool corridor_trace(const SRC &src, const CorridorWin &w, const CorridorRule &r, const int *p, const int *q, unsigned long long &rec0,
                                      unsigned long long &rec1, int &count, int &ex, int &ey, int &ez, int &fx, int &fy, int &fz) {
  const int lane = threadIdx.x & 63;
  const double a[3] = {(double)p[0] + 0.5, (double)p[1] + 0.5, (double)p[2] + 0.5};
  const double b[3] = {(double)q[0] + 0.5, (double)q[1] + 0.5, (double)q[2] + 0.5};
  rec0 = rec1 = 0ull;
  int mx = 0, my = 0, mz = 0;      // this lane's voxel of the batch
  int lx = p[0], ly = p[1], lz = p[2];  // the voxel emitted before
  bool ok = true;
  int n = 0;
  dda_walk<false, false>(a, b, nullptr, nullptr, [&](int x, int y, int z, int k, bool last) -> bool {
    if (k > 0 && k <= kCorridorManhattan) {
      const unsigned long long ax = x != lx ? 0ull : (y != ly ? 1ull : 2ull);
      const int slot = (k & 63) * 2;
      if (lane == (k >> 6)) {
        if (slot < 64)
          rec0 |= ax << slot;
        else
          rec1 |= ax << (slot - 64);
      }
    }
    lx = x, ly = y, lz = z;
    if (lane == (k & 63)) mx = x, my = y, mz = z;
    n = k + 1;
    if ((k & 63) == 63 || last) {
      const bool mine = lane <= (k & 63);
      const bool bad = mine && !corridor_voxel(src, w, r, mx, my, mz);
      const unsigned long long fail = __ballot(bad);
      if (fail) {
        const int fl = __ffsll((long long)fail) - 1;
        fx = __shfl(mx, fl), fy = __shfl(my, fl), fz = __shfl(mz, fl);
        ok = false;
        return true;
      }
    }
    return false;
  });
  count = n, ex = lx, ey = ly, ez = lz;
  return ok;
}
// (slot arithmetic above: step k lives in lane k >> 6, bit pair k & 63 -- pairs 0 .. 31 in rec0, 32 .. 63 in rec1)

__device__ __forceinline__ int corridor_step_axis(unsigned long long rec0, unsigned long long rec1, int k) {
  const int pair = k & 63;
  const unsigned long long word = pair < 32 ? rec0 : rec1;
  const int mine = (int)((word >> ((pair & 31) * 2)) & 3ull);
  return __shfl(mine, k >> 6);
}

// One path: returns the status; every argument and result is wave-uniform.  WRITE: `first` from the scanned offsets.
template <class SRC, bool WRITE>
__device__ __forceinline__ int corridor_path(const SRC &src, const CorridorWin &w, const CorridorRule &r, const CorridorOut &o, const int32_t *wp, int64_t n_wp,
                                    int64_t a, int64_t b, int64_t first, int &nboxes, int &n_chain, int &bseg, int *bvox) {
  const int lane = threadIdx.x & 63;
  nboxes = 0, n_chain = 0, bseg = -1;
  bvox[0] = bvox[1] = bvox[2] = INT32_MIN;
  if (b < a || a < 0 || b > n_wp) return FIESTA_HIP_CORRIDOR_INVALID;
  // every waypoint within +-2^30, every segment at most 4095 voxel steps long
  bool bad = false;
  for (int64_t base = a; base < b; base += 64) {
    const int64_t i = base + lane;
    if (i < b) {
      long long l1 = 0;
      for (int c = 0; c < 3; ++c) {
        const int v = wp[3 * i + c];
        bad = bad || v < -kCorridorCoordMax || v > kCorridorCoordMax;
        if (i + 1 < b) l1 += llabs((long long)wp[3 * (i + 1) + c] - v);
      }
      bad = bad || l1 > kCorridorManhattan;
    }
  }
  if (__ballot(bad)) return FIESTA_HIP_CORRIDOR_INVALID;
  if (a == b) return FIESTA_HIP_CORRIDOR_OK;
  int p[3] = {wp[3 * a], wp[3 * a + 1], wp[3 * a + 2]};
  if (!corridor_voxel(src, w, r, p[0], p[1], p[2])) {  // (every lane tests the same voxel)
    bvox[0] = p[0], bvox[1] = p[1], bvox[2] = p[2];
    return FIESTA_HIP_CORRIDOR_BLOCKED;
  }
  CorridorWalk s;
  s.nboxes = 0, s.idx = 0, s.px = s.py = s.pz = 0;
  int status = FIESTA_HIP_CORRIDOR_OK;
  // j = a - 1 stands for the first waypoint itself: a chain of one voxel.  One visit loop serves every case: a chain is `head`
  // voxels taken as they are (B: the traversal's last voxel if it stopped beside p), `cnt - 1` replayed steps -- each adds the
  // segment's sign on the recorded axis, forwards for A, backwards for B, whose traversal ran the other way -- and `tail` (A: q)
  for (int64_t j = a - 1; j + 1 < b; ++j) {
    const int q[3] = {wp[3 * (j + 1)], wp[3 * (j + 1) + 1], wp[3 * (j + 1) + 2]};
    if (j >= a && q[0] == p[0] && q[1] == p[1] && q[2] == p[2]) continue;
    const int sg[3] = {sgn_i(q[0] - p[0]), sgn_i(q[1] - p[1]), sgn_i(q[2] - p[2])};
    unsigned long long rec0 = 0ull, rec1 = 0ull;
    int cnt = 1, head = 0, tail = 1, c[3] = {p[0], p[1], p[2]};
    bool use_b = false;
    if (j >= a) {
      int ex, ey, ez, fx = 0, fy = 0, fz = 0, gx, gy, gz;
      // candidate A: walk(p, q), then q unless q is its last voxel
      bool ok = corridor_trace(src, w, r, p, q, rec0, rec1, cnt, ex, ey, ez, fx, fy, fz);
      tail = !(ex == q[0] && ey == q[1] && ez == q[2]);
      if (ok && tail && !corridor_voxel(src, w, r, q[0], q[1], q[2])) ok = false, fx = q[0], fy = q[1], fz = q[2];
      if (!ok) {
        // candidate B: the reverse of walk(q, p) followed by p (p itself is traversable: it was visited)
        if (!corridor_trace(src, w, r, q, p, rec0, rec1, cnt, ex, ey, ez, gx, gy, gz)) {
          status = FIESTA_HIP_CORRIDOR_BLOCKED;
          bseg = (int)(j - a);
          bvox[0] = fx, bvox[1] = fy, bvox[2] = fz;
          break;
        }
        use_b = true, tail = 0;
        head = !(ex == p[0] && ey == p[1] && ez == p[2]);
        c[0] = ex, c[1] = ey, c[2] = ez;
      }
    }
    const int total = head + (cnt - 1) + tail;
    for (int t = 0; t < total; ++t) {
      if (t >= head && t < head + cnt - 1) {
        const int ax = corridor_step_axis(rec0, rec1, use_b ? cnt - 1 - (t - head) : t + 1);
        c[0] += ax == 0 ? sg[0] : 0, c[1] += ax == 1 ? sg[1] : 0, c[2] += ax == 2 ? sg[2] : 0;
      } else if (t >= head) {
        c[0] = q[0], c[1] = q[1], c[2] = q[2];
      }
      corridor_visit<SRC, WRITE>(src, w, r, o, first, s, c[0], c[1], c[2]);
    }
    p[0] = q[0], p[1] = q[1], p[2] = q[2];
  }
  nboxes = s.nboxes, n_chain = s.idx;
  return status;
}

template <class SRC>
__global__ __launch_bounds__(kCorridorBlock) void k_corridor_count(SRC src_, CorridorWin w_, CorridorRule r_, CorridorIn in_, CorridorOut o_) {
  const CorridorIn in = corridor_in_vgprs(in_);
  const int32_t *wp = in.wp;
  const int64_t *poff = in.poff;
  const int64_t n_wp = in.n_wp, n = in.n;
  const SRC src = corridor_in_vgprs(src_);
  const CorridorWin w = corridor_in_vgprs(w_);
  const CorridorRule r = corridor_in_vgprs(r_);
  const CorridorOut o = corridor_in_vgprs(o_);
  const int64_t stride = (int64_t)gridDim.x * (kCorridorBlock / 64);
  for (int64_t p = blockIdx.x * (int64_t)(kCorridorBlock / 64) + (threadIdx.x >> 6); p < n; p += stride) {
    int nboxes, n_chain, bseg, bvox[3];
    int st = corridor_path<SRC, false>(src, w, r, o, wp, n_wp, poff[p], poff[p + 1], 0, nboxes, n_chain, bseg, bvox);
    if (st == FIESTA_HIP_CORRIDOR_INVALID) nboxes = 0;
    if ((threadIdx.x & 63) == 0) {
      o.offsets[p + 1] = nboxes;
      if (o.status) o.status[p] = st;
      if (o.n_chain) o.n_chain[p] = n_chain;
      if (o.blocked_segment) o.blocked_segment[p] = bseg;
      if (o.blocked_vox) o.blocked_vox[3 * p] = bvox[0], o.blocked_vox[3 * p + 1] = bvox[1], o.blocked_vox[3 * p + 2] = bvox[2];
    }
  }
}

template <class SRC>
__global__ __launch_bounds__(kCorridorBlock) void k_corridor_write(SRC src_, CorridorWin w_, CorridorRule r_, CorridorIn in_, CorridorOut o_) {
  const CorridorIn in = corridor_in_vgprs(in_);
  const int32_t *wp = in.wp;
  const int64_t *poff = in.poff;
  const int64_t n_wp = in.n_wp, n = in.n;
  const SRC src = corridor_in_vgprs(src_);
  const CorridorWin w = corridor_in_vgprs(w_);
  const CorridorRule r = corridor_in_vgprs(r_);
  const CorridorOut o = corridor_in_vgprs(o_);
  const int64_t stride = (int64_t)gridDim.x * (kCorridorBlock / 64);
  for (int64_t p = blockIdx.x * (int64_t)(kCorridorBlock / 64) + (threadIdx.x >> 6); p < n; p += stride) {
    const int64_t first = o.offsets[p], count = o.offsets[p + 1] - first;
    if (count <= 0 || first >= o.capacity) continue;  // no box, or all of them beyond the capacity
    int nboxes, n_chain, bseg, bvox[3];
    (void)corridor_path<SRC, true>(src, w, r, o, wp, n_wp, poff[p], poff[p + 1], first, nboxes, n_chain, bseg, bvox);
  }
}

inline int corridor_blocks(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + 3) / 4, kCorridorMaxBlocks)); }

// Both call pairs on a map's stream.  w: the window as the store sees it (resolution and origin included).  The device variants only
// enqueue; the host variants stage through P.in / P.out and synchronise (the corridor call reads the totals back between the count
// and the write pass, so that it stages min(total, capacity) boxes).
template <class SRC>
void corridor_run(hipStream_t st, PlannerScratch &P, const SRC &src, const CorridorWin &w, const CorridorArgs &a) {
  const CorridorRule rule{a.min_clearance, (a.flags & FIESTA_HIP_CORRIDOR_THROUGH_UNKNOWN) ? 1 : 0, a.max_grow};
  if (!a.paths) {
    const int64_t n = a.n_vox;
    if (n <= 0) return;
    const fiesta_hip_free_boxes_result &r = *a.boxes;
    if (a.dev) {
      hipLaunchKernelGGL(k_free_boxes<SRC>, dim3(corridor_blocks(n)), dim3(kCorridorBlock), 0, st, src, w, rule, a.vox, n,
                         FreeBoxOut{r.box, r.box_pos, r.stop, r.volume, r.status});
      FIESTA_HIP_CHECK(hipGetLastError());
      return;
    }
    const size_t cnt = (size_t)n;
    Staging in{P.in, st}, out{P.out, st};
    const auto seeds = in.add(a.vox, 3 * cnt);
    in.alloc(), in.up(seeds, 3 * cnt);
    const auto pos = out.add(r.box_pos, 6 * cnt);
    const auto vol = out.add(r.volume, cnt);
    const auto box = out.add(r.box, 6 * cnt);
    const auto status = out.add(r.status, cnt);
    const auto stop = out.add(r.stop, 6 * cnt);
    out.alloc();
    hipLaunchKernelGGL(k_free_boxes<SRC>, dim3(corridor_blocks(n)), dim3(kCorridorBlock), 0, st, src, w, rule, (const int32_t *)in.dev(seeds), n,
                       FreeBoxOut{out.dev(box), out.dev(pos), out.dev(stop), out.dev(vol), out.dev(status)});
    FIESTA_HIP_CHECK(hipGetLastError());
    out.back(pos, 6 * cnt), out.back(vol, cnt), out.back(box, 6 * cnt), out.back(status, cnt), out.back(stop, 6 * cnt);
    FIESTA_HIP_CHECK(hipStreamSynchronize(st));
    return;
  }
  const fiesta_hip_corridor_result &r = *a.corridor;
  const int64_t n = a.n_paths;
  if (a.dev) {
    const CorridorOut o{r.offsets, r.boxes, r.boxes_pos, r.stop, r.entry, r.status, r.n_chain, r.blocked_segment, r.blocked_vox, a.capacity};
    if (n > 0) {
      hipLaunchKernelGGL(k_corridor_count<SRC>, dim3(corridor_blocks(n)), dim3(kCorridorBlock), 0, st, src, w, rule, CorridorIn{a.vox, a.n_vox, a.offsets, n}, o);
      FIESTA_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_reach_path_scan, dim3(1), dim3(256), 0, st, r.offsets, n);
    FIESTA_HIP_CHECK(hipGetLastError());
    if (n > 0 && a.capacity > 0 && (r.boxes || r.boxes_pos || r.stop || r.entry)) {
      hipLaunchKernelGGL(k_corridor_write<SRC>, dim3(corridor_blocks(n)), dim3(kCorridorBlock), 0, st, src, w, rule, CorridorIn{a.vox, a.n_vox, a.offsets, n}, o);
      FIESTA_HIP_CHECK(hipGetLastError());
    }
    return;
  }
  if (n == 0) {
    r.offsets[0] = 0;
    return;
  }
  const size_t cnt = (size_t)n, nw = (size_t)a.n_vox;
  Staging in{P.in, st}, out{P.out, st};
  const auto poff = in.add(a.offsets, cnt + 1);
  const auto wp = in.add(a.vox, 3 * nw);
  in.alloc(), in.up(poff, cnt + 1), in.up(wp, 3 * nw);
  const auto offsets = out.add(r.offsets, cnt + 1);
  const auto status = out.add(r.status, cnt), n_chain = out.add(r.n_chain, cnt), bseg = out.add(r.blocked_segment, cnt);
  const auto bvox = out.add(r.blocked_vox, 3 * cnt);
  const size_t head = out.end;
  out.alloc();
  CorridorOut o{out.dev(offsets), nullptr, nullptr, nullptr, nullptr, out.dev(status), out.dev(n_chain), out.dev(bseg), out.dev(bvox), 0};
  hipLaunchKernelGGL(k_corridor_count<SRC>, dim3(corridor_blocks(n)), dim3(kCorridorBlock), 0, st, src, w, rule,
                     CorridorIn{in.dev(wp), a.n_vox, in.dev(poff), n}, o);
  FIESTA_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_reach_path_scan, dim3(1), dim3(256), 0, st, o.offsets, n);
  FIESTA_HIP_CHECK(hipGetLastError());
  out.back(offsets, cnt + 1), out.back(status, cnt), out.back(n_chain, cnt), out.back(bseg, cnt), out.back(bvox, 3 * cnt);
  FIESTA_HIP_CHECK(hipStreamSynchronize(st));
  const int64_t nb = std::min<int64_t>(r.offsets[n], a.capacity);
  if (nb <= 0 || (!r.boxes && !r.boxes_pos && !r.stop && !r.entry)) return;
  const auto pos = out.add(r.boxes_pos, 6 * (size_t)nb);
  const auto boxes = out.add(r.boxes, 6 * (size_t)nb);
  const auto entry = out.add(r.entry, (size_t)nb);
  const auto stop = out.add(r.stop, 6 * (size_t)nb);
  out.alloc(head);  // (the buffer may move; the scanned offsets are kept: the write pass reads them)
  o = CorridorOut{out.dev(offsets), out.dev(boxes), out.dev(pos), out.dev(stop), out.dev(entry), nullptr, nullptr, nullptr, nullptr, nb};
  hipLaunchKernelGGL(k_corridor_write<SRC>, dim3(corridor_blocks(n)), dim3(kCorridorBlock), 0, st, src, w, rule,
                     CorridorIn{in.dev(wp), a.n_vox, in.dev(poff), n}, o);
  FIESTA_HIP_CHECK(hipGetLastError());
  out.back(pos, 6 * (size_t)nb), out.back(boxes, 6 * (size_t)nb), out.back(entry, (size_t)nb), out.back(stop, 6 * (size_t)nb);
  FIESTA_HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace
}  // namespace fiesta
