// fiesta_amd/csrc/reach_kernels.hpp -- reachability: fiesta_hip_reach_field / _dev (include/fiesta_hip.h).
//
// A planner asks "which of these places can the robot reach from here, and how far is it?": a shortest-path flood over the
// TRAVERSABLE voxels of a box (observed free, optionally with a clearance, optionally the never-observed ones too) with the 3-4-5
// chamfer weights.  The flood is the relaxation engine's pattern (relax_kernels.hpp) over traversability instead of obstacle ids:
//   k_reach_mask<SRC>    the only kernel that knows the map: one lane per 32-voxel z-word of the box builds the box-local
//                        traversability bitmap (SRC::row: observed and occupied bits of 32 voxels from any z, so an unaligned box
//                        origin is two source words and a funnel shift; the clearance filter is frontier_filter, the frontier call's),
//                        initialises the cost field (-1 / INT32_MAX, whole cache lines per half wave) and counts the traversable voxels
//   k_reach_seed         usable seeds get cost 0 and wake their tiles
//   k_reach_relax<CONN>  one work-group per ACTIVE tile (16 x 16 x 32 voxels of the box): costs + 1-voxel halo in LDS (18 x 18 x 34
//                        i32, 43 KiB), every lane owns one z-column and PULLS min(own, neighbour + w) until a whole sweep between two
//                        barriers changes nothing; only changed costs go back, and a changed outermost layer wakes the tile behind it
//   k_reach_targets / k_reach_stats   the finishing pass: the targets' costs; reached voxels and the largest cost
// Rounds are separate launches over a list of active tiles (flags and lists double-buffered by round parity, their lengths rotate
// through three counters so that nothing is cleared between rounds); an empty list exits at once.  The host enqueues kReachChain
// rounds, then reads the counters once.  No cooperative launch, no waiting of one work-group for another.
// All arithmetic is integer (the clearance comparison apart); the fixed point of a shortest-path relaxation on integer weights is
// unique, so every output is the same for any launch shape and scheduling.
#pragma once
#include <algorithm>
#include <climits>

#include "../../include/fiesta_hip.h"
#include "common.hpp"
#include "planner.hpp"
#include "planner_args.hpp"
#include "frontier_kernels.hpp"
#include "relax_kernels.hpp"

namespace fiesta {
namespace {  // (planner.hip alone includes this header; the namespace is part of the kernels' symbol names)

constexpr int kReachBig = INT32_MAX - 8;        // "no cost yet" inside LDS: kReachBig + 5 does not overflow, real costs stay below it
constexpr int kReachPitchZ = 34, kReachPitchY = 18 * 34, kReachLds = 18 * 18 * 34;
constexpr int kReachChain = 8;                  // rounds enqueued between two reads of the counters
constexpr int kReachMaxGroups = 768;            // relaxation work-groups per round (3 per CU by their LDS); longer lists stride

enum ReachCounter { R_LIST0 = 0, R_LIST1, R_LIST2, R_NTRAV, R_SEEDS, R_ROUNDS, R_VISITS, R_REACHED, R_MAXCOST, R_COUNT };

struct ReachBox {
  int sx0, sy0, sz0;  // the coordinates SRC takes for box voxel (0, 0, 0)
  int ex, ey, ez;     // extents; ex * ey * ez <= 2^28
  int nzw;            // 32-voxel words per z-row of the box = tiles along z
  int ntx, nty;       // tiles along x and y
};
struct ReachRound {
  uint32_t *flag_cur, *flag_next;  // per tile: queued for this round / the next one
  const uint32_t *list_cur;
  uint32_t *list_next;
  unsigned long long *ctr;
  int cur, next, clear;  // R_LIST*: this round's length, the next round's, the one to zero (consumed by the round before)
};

// SRC: void row(int x, int y, int z0, uint32_t &obs, uint32_t &occ) -- observed / occupied bits of voxels (x, y, z0 + k), k < 32 (no
//      voxel there: both 0) -- and double operator()(int x, int y, int z): GetDistance(Vector3i) of that voxel (frontier_filter's DIST)
template <class SRC>
__global__ __launch_bounds__(256) void k_reach_mask(SRC src, ReachBox b, double min_clearance, int through_unknown, uint32_t *bits,
                                                    int32_t *cost, unsigned long long *ctr) {
  const int lane = threadIdx.x & 63;
  const int n = b.ex * b.ey * b.nzw;
  // (the trip count is the same for every lane of the work-group: the shuffles below need whole waves)
  for (int base = blockIdx.x * 256; base < n; base += gridDim.x * 256) {
    const int i = base + threadIdx.x;
    uint32_t t = 0;
    int cb = 0, nv = 0;
    if (i < n) {
      const int w = i % b.nzw, row = i / b.nzw, y = row % b.ey, x = row / b.ey;
      nv = min(32, b.ez - 32 * w);  // (the last word of a row may be short: its upper bits are no voxels of the box)
      const uint32_t valid = nv == 32 ? 0xFFFFFFFFu : ((1u << nv) - 1u);
      const int sx = b.sx0 + x, sy = b.sy0 + y, sz = b.sz0 + 32 * w;
      uint32_t obs, occ;
      src.row(sx, sy, sz, obs, occ);
      uint32_t fre = obs & ~occ & valid;
      if (fre && min_clearance > 0) fre = frontier_filter(src, fre, sx, sy, sz, min_clearance);
      t = fre | (through_unknown ? (~obs & valid) : 0u);
      bits[i] = t;
      cb = row * b.ez + 32 * w;
    }
    // the costs of this wave's 64 words, two words per store instruction: 32 consecutive i32 per half wave
    for (int j = 0; j < 32; ++j) {
      const int from = 2 * j + (lane >> 5), k = lane & 31;
      const uint32_t tw = (uint32_t)__shfl((int)t, from);
      const int c = __shfl(cb, from), v = __shfl(nv, from);
      if (k < v) cost[c + k] = ((tw >> k) & 1u) ? INT32_MAX : -1;
    }
    const int cnt = wave_sum(__popc(t));
    if (lane == 0 && cnt) atomicAdd(&ctr[R_NTRAV], (unsigned long long)cnt);
  }
}

// (ox, oy, oz): map voxel of box voxel (0, 0, 0)
__global__ __launch_bounds__(256) void k_reach_seed(ReachBox b, int ox, int oy, int oz, const int32_t *seeds, int64_t n, const uint32_t *bits,
                                                    int32_t *cost, uint32_t *flag, uint32_t *list, unsigned long long *ctr) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t x = (int64_t)seeds[3 * i] - ox, y = (int64_t)seeds[3 * i + 1] - oy, z = (int64_t)seeds[3 * i + 2] - oz;
  bool usable = x >= 0 && x < b.ex && y >= 0 && y < b.ey && z >= 0 && z < b.ez;
  if (usable) usable = (bits[((int)x * b.ey + (int)y) * b.nzw + ((int)z >> 5)] >> ((int)z & 31)) & 1u;
  if (usable) {
    cost[((int64_t)x * b.ey + y) * b.ez + z] = 0;
    activate_tile((uint32_t)((((int)x >> 4) * b.nty + ((int)y >> 4)) * b.nzw + ((int)z >> 5)), flag, list, &ctr[R_LIST0]);
  }
  const unsigned long long m = __ballot(usable);
  if (m && (int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(&ctr[R_SEEDS], (unsigned long long)__popcll(m));
}

// One round.  Why the unsynchronised halo is safe: a tile's halo cells are the outermost layers of its neighbours, which other
// work-groups of the SAME round may be writing back while this one stages them.  An aligned 32-bit load returns the old or the new
// value (possibly the old one from a cache the writer does not share); every value ever stored is the weight of a real move
// sequence from a seed, so both are upper bounds of the final cost and min() over upper bounds never goes below it.  A neighbour
// that lowers such a layer wakes this tile for the NEXT round -- a later launch, which sees everything this launch wrote -- so no
// improvement is lost; and since a wake-up for round r + 1 goes to the flags and the list of the other parity, it cannot be erased
// by the tile clearing its own flag of round r.  The same holds inside LDS between the lanes of one sweep: the loop ends only after
// a sweep in which, between two barriers, no lane changed anything, i.e. every lane has seen the final values of its neighbours.
//
// The visit of one tile by one work-group of 256 lanes, shared by k_reach_relax and the batched floods of reach_matrix_kernels.hpp
// (k_rmx_relax): `cost` is the field (there: the flood's own plane), `t` the tile, and `item0` what the flags and lists add to a
// tile index (0 here; there flood * ntiles, so that a lowered outer layer wakes the neighbouring tile OF THE SAME FLOOD).
template <int CONN>
__device__ __forceinline__ void reach_relax_tile(const ReachBox &b, const uint32_t *bits, int32_t *cost, const ReachRound &r, int t, uint32_t item0) {
  __shared__ int s_c[kReachLds];
  __shared__ int s_wake[27];
  const int tid = threadIdx.x, lx = tid >> 4, ly = tid & 15;
  const int tz = t % b.nzw, ty = (t / b.nzw) % b.nty, tx = t / (b.nzw * b.nty);
  if (tid == 0) r.flag_cur[item0 + (uint32_t)t] = 0;
  if (tid < 27) s_wake[tid] = 0;
  for (int i = tid; i < kReachLds; i += 256) {
    const int hz = i % 34, hy = (i / 34) % 18, hx = i / kReachPitchY;
    const int x = tx * 16 - 1 + hx, y = ty * 16 - 1 + hy, z = tz * 32 - 1 + hz;
    int v = kReachBig;  // outside the box, not traversable, not reached: nothing to pull from
    if ((unsigned)x < (unsigned)b.ex && (unsigned)y < (unsigned)b.ey && (unsigned)z < (unsigned)b.ez) {
      const int c = cost[((int64_t)x * b.ey + y) * b.ez + z];
      if (c >= 0 && c != INT32_MAX) v = c;
    }
    s_c[i] = v;
  }
  const int x = tx * 16 + lx, y = ty * 16 + ly;
  const uint32_t own = (x < b.ex && y < b.ey) ? bits[(x * b.ey + y) * b.nzw + tz] : 0u;  // this lane's column: one word
  const int base = (lx + 1) * kReachPitchY + (ly + 1) * kReachPitchZ + 1;
  __syncthreads();
  uint32_t chg = 0;  // voxels of the column whose cost this visit lowered
  for (int sweep = 0;; ++sweep) {
    bool ch = false;
    for (uint32_t m = own; m;) {  // (a word without traversable voxels is skipped) upwards and downwards in turn
      const int z = (sweep & 1) ? 31 - __clz((int)m) : __ffs((int)m) - 1;
      m &= ~(1u << z);
      const int p = base + z, cur = s_c[p];
      int best = cur;
#define FIESTA_REACH_PULL(DX, DY, DZ, W) best = min(best, s_c[p + (DX) * kReachPitchY + (DY) * kReachPitchZ + (DZ)] + (W));
      FIESTA_REACH_PULL(0, 0, -1, 3) FIESTA_REACH_PULL(0, 0, 1, 3) FIESTA_REACH_PULL(-1, 0, 0, 3) FIESTA_REACH_PULL(1, 0, 0, 3)
      FIESTA_REACH_PULL(0, -1, 0, 3) FIESTA_REACH_PULL(0, 1, 0, 3)
      if (CONN == 26) {
        FIESTA_REACH_PULL(-1, -1, 0, 4) FIESTA_REACH_PULL(-1, 1, 0, 4) FIESTA_REACH_PULL(1, -1, 0, 4) FIESTA_REACH_PULL(1, 1, 0, 4)
        FIESTA_REACH_PULL(-1, 0, -1, 4) FIESTA_REACH_PULL(-1, 0, 1, 4) FIESTA_REACH_PULL(1, 0, -1, 4) FIESTA_REACH_PULL(1, 0, 1, 4)
        FIESTA_REACH_PULL(0, -1, -1, 4) FIESTA_REACH_PULL(0, -1, 1, 4) FIESTA_REACH_PULL(0, 1, -1, 4) FIESTA_REACH_PULL(0, 1, 1, 4)
        FIESTA_REACH_PULL(-1, -1, -1, 5) FIESTA_REACH_PULL(-1, -1, 1, 5) FIESTA_REACH_PULL(-1, 1, -1, 5) FIESTA_REACH_PULL(-1, 1, 1, 5)
        FIESTA_REACH_PULL(1, -1, -1, 5) FIESTA_REACH_PULL(1, -1, 1, 5) FIESTA_REACH_PULL(1, 1, -1, 5) FIESTA_REACH_PULL(1, 1, 1, 5)
      }
#undef FIESTA_REACH_PULL
      if (best < cur) s_c[p] = best, ch = true, chg |= 1u << z;
    }
    if (!__syncthreads_or(ch)) break;
  }
  const int64_t gi = ((int64_t)x * b.ey + y) * b.ez + tz * 32;
  for (uint32_t m = chg; m; m &= m - 1) {
    const int z = __ffs((int)m) - 1;
    cost[gi + z] = s_c[base + z];
  }
  // a lowered cost in the layer that faces a neighbouring tile (a face, an edge, a corner) is news for that tile
#pragma unroll
  for (int d = 0; d < 27; ++d) {
    const int dx = d / 9 - 1, dy = (d / 3) % 3 - 1, dz = d % 3 - 1;
    if (d == 13 || (CONN == 6 && (dx != 0) + (dy != 0) + (dz != 0) != 1)) continue;
    const bool layer = (dx == 0 || lx == (dx < 0 ? 0 : 15)) && (dy == 0 || ly == (dy < 0 ? 0 : 15));
    const uint32_t zm = dz == 0 ? 0xFFFFFFFFu : (dz < 0 ? 1u : 0x80000000u);
    if (layer && (chg & zm)) s_wake[d] = 1;
  }
  __syncthreads();
  if (tid < 27 && s_wake[tid]) {
    const int ux = tx + tid / 9 - 1, uy = ty + (tid / 3) % 3 - 1, uz = tz + tid % 3 - 1;
    if (ux >= 0 && ux < b.ntx && uy >= 0 && uy < b.nty && uz >= 0 && uz < b.nzw)
      activate_tile(item0 + (uint32_t)((ux * b.nty + uy) * b.nzw + uz), r.flag_next, r.list_next, &r.ctr[r.next]);
  }
  if (tid == 0) atomicAdd(&r.ctr[R_VISITS], 1ull);
  __syncthreads();  // (the next tile overwrites s_c and s_wake)
}

template <int CONN>
__global__ __launch_bounds__(256) void k_reach_relax(ReachBox b, const uint32_t *bits, int32_t *cost, ReachRound r) {
  const unsigned count = (unsigned)r.ctr[r.cur];  // (nothing appends to this round's own list)
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    r.ctr[r.clear] = 0;
    if (count) atomicAdd(&r.ctr[R_ROUNDS], 1ull);
  }
  for (unsigned it = blockIdx.x; it < count; it += gridDim.x) reach_relax_tile<CONN>(b, bits, cost, r, (int)r.list_cur[it], 0u);
}

__global__ __launch_bounds__(256) void k_reach_targets(ReachBox b, int ox, int oy, int oz, const int32_t *targets, int64_t n, const int32_t *cost,
                                                       int32_t *out) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t x = (int64_t)targets[3 * i] - ox, y = (int64_t)targets[3 * i + 1] - oy, z = (int64_t)targets[3 * i + 2] - oz;
  const bool in = x >= 0 && x < b.ex && y >= 0 && y < b.ey && z >= 0 && z < b.ez;
  out[i] = in ? cost[(x * b.ey + y) * b.ez + z] : -1;
}

__global__ __launch_bounds__(256) void k_reach_stats(const int32_t *cost, int64_t n, unsigned long long *ctr) {
  int cnt = 0, mx = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = cost[i];
    if (c >= 0 && c != INT32_MAX) ++cnt, mx = max(mx, c);
  }
  cnt = wave_sum(cnt), mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0 && cnt) {
    atomicAdd(&ctr[R_REACHED], (unsigned long long)cnt);
    atomicMax(&ctr[R_MAXCOST], (unsigned long long)mx);
  }
}

__global__ void k_reach_fill(int32_t *out, int64_t n, int32_t v) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < n) out[i] = v;
}

inline int reach_blocks(int64_t n, int per, int cap) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + per - 1) / per, cap)); }

// Both variants of the call on a map's stream.  lo / hi: the clipped box in SRC's coordinates (lo[c] > hi[c]: empty); off: what
// turns them into map voxel coordinates.  Both variants synchronise: the number of rounds depends on the data.
template <class SRC>
void reach_run(hipStream_t st, PlannerScratch &P, const SRC &src, const int64_t lo[3], const int64_t hi[3], const int off[3], const ReachArgs &a) {
  ReachScratch &S = P.reach;
  DevBuf<unsigned char> &in = P.in, &out = P.out;  // the staged seeds and targets; the staged target costs
  const fiesta_hip_reach_result &res = *a.res;
  S.field_valid = false;  // (fiesta_hip_reach_paths' retained field: only a call that finishes with its costs in S.cost leaves one)
  if (a.info) *a.info = fiesta_hip_reach_info{};
  const bool want_targets = res.target_cost && a.n_targets > 0;
  int32_t *dtc = nullptr;
  if (want_targets) {
    if (a.dev)
      dtc = res.target_cost;
    else
      out.ensure((size_t)a.n_targets * sizeof(int32_t), st), dtc = (int32_t *)out.p;
  }
  auto targets_back = [&] {
    if (want_targets && !a.dev)
      FIESTA_HIP_CHECK(hipMemcpyAsync(res.target_cost, dtc, (size_t)a.n_targets * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  };
  if (lo[0] > hi[0] || lo[1] > hi[1] || lo[2] > hi[2]) {  // nothing to flood: no voxel, every target outside
    if (want_targets) {
      hipLaunchKernelGGL(k_reach_fill, dim3((unsigned)((a.n_targets + 255) / 256)), dim3(256), 0, st, dtc, a.n_targets, -1);
      FIESTA_HIP_CHECK(hipGetLastError());
    }
    targets_back();
    FIESTA_HIP_CHECK(hipStreamSynchronize(st));
    return;
  }
  const int64_t ex = hi[0] - lo[0] + 1, ey = hi[1] - lo[1] + 1, ez = hi[2] - lo[2] + 1;
  // (each extent is below 2^32, so the first product cannot overflow before it is tested)
  if (ex > kReachMaxVoxels || ey > kReachMaxVoxels || ex * ey > kReachMaxVoxels || ex * ey * ez > kReachMaxVoxels)
    throw Error(FIESTA_HIP_ERR_INVALID, "reach_field: the clipped box holds more than 2^28 voxels");
  const int64_t nvox = ex * ey * ez;
  ReachBox b{(int)lo[0], (int)lo[1], (int)lo[2], (int)ex, (int)ey, (int)ez, (int)((ez + 31) / 32), (int)((ex + 15) / 16), (int)((ey + 15) / 16)};
  const int64_t nwords = ex * ey * b.nzw, ntiles = (int64_t)b.ntx * b.nty * b.nzw;
  const int ox = (int)(lo[0] + off[0]), oy = (int)(lo[1] + off[1]), oz = (int)(lo[2] + off[2]);
  // scratch, owned by the map (an allocation failure is FIESTA_HIP_ERR_NOMEM and leaves what there was)
  S.bits.ensure_exact((size_t)nwords, st);
  S.flags.ensure((size_t)(2 * ntiles), st);
  S.lists.ensure((size_t)(2 * ntiles), st);
  S.ctr.ensure(R_COUNT, st);
  int32_t *dcost = (a.dev && res.cost) ? res.cost : nullptr;
  if (!dcost) S.cost.ensure_exact((size_t)nvox, st), dcost = S.cost.p;
  const int32_t *dseeds = a.seeds, *dtargets = a.targets;
  if (!a.dev) {
    const size_t sb = (size_t)a.n_seeds * 3 * sizeof(int32_t), tb = want_targets ? (size_t)a.n_targets * 3 * sizeof(int32_t) : 0;
    in.ensure(sb + tb + 8, st);
    if (sb) FIESTA_HIP_CHECK(hipMemcpyAsync(in.p, a.seeds, sb, hipMemcpyHostToDevice, st));
    if (tb) FIESTA_HIP_CHECK(hipMemcpyAsync(in.p + sb, a.targets, tb, hipMemcpyHostToDevice, st));
    dseeds = (const int32_t *)in.p, dtargets = (const int32_t *)(in.p + sb);
  }
  FIESTA_HIP_CHECK(hipMemsetAsync(S.ctr.p, 0, R_COUNT * sizeof(unsigned long long), st));
  FIESTA_HIP_CHECK(hipMemsetAsync(S.flags.p, 0, (size_t)(2 * ntiles) * sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_reach_mask<SRC>, dim3(reach_blocks(nwords, 256, 8192)), dim3(256), 0, st, src, b, a.min_clearance,
                     (a.flags & FIESTA_HIP_REACH_THROUGH_UNKNOWN) ? 1 : 0, S.bits.p, dcost, S.ctr.p);
  FIESTA_HIP_CHECK(hipGetLastError());
  uint32_t *flag[2] = {S.flags.p, S.flags.p + ntiles}, *list[2] = {S.lists.p, S.lists.p + ntiles};
  if (a.n_seeds > 0) {
    hipLaunchKernelGGL(k_reach_seed, dim3((unsigned)((a.n_seeds + 255) / 256)), dim3(256), 0, st, b, ox, oy, oz, dseeds, a.n_seeds,
                       (const uint32_t *)S.bits.p, dcost, flag[0], list[0], S.ctr.p);
    FIESTA_HIP_CHECK(hipGetLastError());
  }
  unsigned long long h[R_COUNT];
  auto read_counters = [&] {
    FIESTA_HIP_CHECK(hipMemcpyAsync(h, S.ctr.p, sizeof(h), hipMemcpyDeviceToHost, st));
    FIESTA_HIP_CHECK(hipStreamSynchronize(st));
  };
  const int groups = (int)std::min<int64_t>(ntiles, kReachMaxGroups);
  for (int64_t round = 0;;) {
    if (a.n_seeds > 0)
      for (int k = 0; k < kReachChain; ++k, ++round) {
        const int p = (int)(round & 1);
        const ReachRound rr{flag[p], flag[p ^ 1], list[p], list[p ^ 1], S.ctr.p, R_LIST0 + (int)(round % 3), R_LIST0 + (int)((round + 1) % 3),
                            R_LIST0 + (int)((round + 2) % 3)};
        if (a.connectivity == 6)
          hipLaunchKernelGGL(k_reach_relax<6>, dim3(groups), dim3(256), 0, st, b, (const uint32_t *)S.bits.p, dcost, rr);
        else
          hipLaunchKernelGGL(k_reach_relax<26>, dim3(groups), dim3(256), 0, st, b, (const uint32_t *)S.bits.p, dcost, rr);
        FIESTA_HIP_CHECK(hipGetLastError());
      }
    read_counters();
    if (a.n_seeds <= 0 || h[R_LIST0 + round % 3] == 0) break;
    // after round r every voxel whose shortest path crosses fewer than r tile faces is final: more rounds than voxels is a bug
    if (h[R_ROUNDS] > h[R_NTRAV] + 1) throw Error(FIESTA_HIP_ERR_STATE, "reach_field: the flood did not settle");
  }
  if (want_targets) {
    hipLaunchKernelGGL(k_reach_targets, dim3((unsigned)((a.n_targets + 255) / 256)), dim3(256), 0, st, b, ox, oy, oz, dtargets, a.n_targets,
                       (const int32_t *)dcost, dtc);
    FIESTA_HIP_CHECK(hipGetLastError());
  }
  if (a.info) {
    hipLaunchKernelGGL(k_reach_stats, dim3(reach_blocks(nvox, 256 * 16, 2048)), dim3(256), 0, st, (const int32_t *)dcost, nvox, S.ctr.p);
    FIESTA_HIP_CHECK(hipGetLastError());
  }
  targets_back();
  if (res.cost && !a.dev) FIESTA_HIP_CHECK(hipMemcpyAsync(res.cost, dcost, (size_t)nvox * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (a.info) {
    read_counters();
    fiesta_hip_reach_info &I = *a.info;
    I.box_lo[0] = ox, I.box_lo[1] = oy, I.box_lo[2] = oz;
    I.box_hi[0] = (int32_t)(hi[0] + off[0]), I.box_hi[1] = (int32_t)(hi[1] + off[1]), I.box_hi[2] = (int32_t)(hi[2] + off[2]);
    I.n_traversable = (int64_t)h[R_NTRAV], I.n_seeds_used = (int64_t)h[R_SEEDS], I.n_reached = (int64_t)h[R_REACHED];
    I.max_cost = (int64_t)h[R_MAXCOST], I.rounds = (int64_t)h[R_ROUNDS], I.tile_visits = (int64_t)h[R_VISITS];
  } else {
    FIESTA_HIP_CHECK(hipStreamSynchronize(st));
  }
  if (dcost == S.cost.p) {
    S.field_lo[0] = ox, S.field_lo[1] = oy, S.field_lo[2] = oz;
    for (int c = 0; c < 3; ++c) S.field_hi[c] = (int32_t)(hi[c] + off[c]);
    S.field_connectivity = a.connectivity;
    S.field_valid = true;
  }
}

}  // namespace
}  // namespace fiesta
