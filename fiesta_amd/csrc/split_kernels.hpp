// fiesta_amd/csrc/split_kernels.hpp -- bisect large clusters into view-sized parts: fiesta_hip_split_clusters / _dev (include/fiesta_hip.h).
//
// The step between fiesta_hip_cluster_voxels and fiesta_hip_view_coverage: frontier surfaces touch, so one cluster can hold most of
// a frontier, and a ring of views around its centroid looks at nothing.  The call cuts every OVERSIZE part of a cluster (more than
// max_size members, or a box longer than max_extent) at the middle of its box's longest axis, level by level, until no part is
// oversize or max_depth is reached.  It reads nothing of a map but its resolution and origin; everything is integer arithmetic but
// the centroids (k_cluster_finish's expression).  The members of a part are always contiguous in a member buffer of the input's
// positions, and a split is a stable partition INSIDE the part's range: nothing else moves.  Passes, all on the map's stream, none
// cooperative, no work-group ever waits for another (the kernel boundary is the only ordering):
//   k_split_init      counters 0, member flags 0, label = -1
//   k_split_validate  ONE validation pass: offsets, member indices, the members' coordinates; a data error sets a device flag that
//                     every later kernel tests first -- they all return, k_split_info reports INVALID
//   k_split_seed      a lane per cluster: a head flag at the first member of every non-empty segment, then one scan (below) numbers
//   k_split_first     the depth-0 parts: a lane per member copies its index and takes its part
//   per level L < max_depth (the host enqueues all of them; a level without an oversize part returns at once on a device counter):
//   k_split_box       a lane per member of a depth-L part: box min / max into per-part words, aggregated inside the wave first
//                     (the members of a part are contiguous: a wave touches few parts; VoxelBox of wave_ops.hpp), and over the 16
//                     chunks a wave takes in a row; a word that already covers the wave's box gets no atomic
//   k_split_decide    a lane per part: oversize? then the axis (largest extent, lowest axis among equals) and mid; counts the cuts
//   k_split_partial   a lane per member: one flag byte -- bit 0: on the high side of its part's cut, bit 1: first member of a part
//                     that is cut -- and the work-group's sum of both counts packed into one 64-bit word (heads high, highs low)
//   k_split_scan      ONE work-group over the <= 8192 partials (an exclusive scan in place); the next level's part count
//   k_split_rescan    a local rescan of every work-group's share from its partial: the exclusive scan per member
//   k_split_scatter   a lane per member: the new part index is the old one plus the cut parts before it (plus one on the high
//                     side); the new position is the part's start plus the rank on its side; written into the OTHER member buffer
//   after the last level:
//   k_split_acc_init / k_split_stats / k_split_finish / k_split_info   per-part sums, box, mask OR, packed (key, index) minimum,
//                     root and the labels with the wave aggregation of wave_ops.hpp (VoxelStats), then voxel_stats_write
// The member scan is reduce-then-scan: no decoupled look-back, no single striding work-group.  Every loop is bounded by a count the
// host passed.  Every quantity is a commutative exact integer reduction and the partition is stable: all outputs but the order
// inside a member segment are the same bits for any launch shape, and the bits of fiesta_amd.split_model.  No scratch memory.
#pragma once
#include <algorithm>
#include <climits>

#include "../../include/fiesta_hip.h"
#include "cluster_kernels.hpp"
#include "common.hpp"
#include "planner.hpp"
#include "planner_args.hpp"

namespace fiesta {
namespace {  // (planner.hip alone includes this header; the namespace is part of the kernels' symbol names)

constexpr int kSplitBlock = 256, kSplitItems = 8, kSplitTile = kSplitBlock * kSplitItems;  // a work-group's share of the member scan
constexpr int kSplitScanBlock = 1024;
constexpr int kSplitBoxRun = 16;  // chunks of 64 members a wave of the box pass takes in a row
constexpr int kSplitLevels = FIESTA_HIP_SPLIT_MAX_DEPTH + 1;
// the counter words (unsigned long long each)
constexpr int kSplitBad = 0, kSplitM0 = 1, kSplitM1 = 2, kSplitK = 3, kSplitLargest = 4, kSplitOver = 5, kSplitCutClusters = 6, kSplitDeepest = 7,
              kSplitCur = 8,                         // [level]: which of the two buffer sets holds the parts when level `level` starts
              kSplitParts = kSplitCur + kSplitLevels + 1,   // [level]: how many parts there are then
              kSplitCuts = kSplitParts + kSplitLevels + 1,  // [level]: parts cut at that level
              kSplitWords = kSplitCuts + kSplitLevels + 1;

// device view of the map's SplitScratch for one call.  M: the member capacity (n_members); T: M rounded up to whole tiles
struct SplitWork {
  int32_t *mem[2], *part[2];           // M each: the member's entry index and its part, by position
  int32_t *start[2], *par[2], *dep[2];  // per part: first position (P + 1 entries), input cluster, depth
  int32_t *box;                        // 6 M: min x, y, z, max x, y, z
  int32_t *axis, *mid;                 // per part: the cut of the level (axis -1: none); seed: the cluster of a head position
  int32_t *proot;                      // per part
  uint32_t *mor;                       // per part
  uint8_t *flags;                      // T
  unsigned long long *pre;             // T + 1: exclusive scan of the flags, heads << 32 | highs
  unsigned long long *partial;         // T / tile + 1
  unsigned long long *sum;             // 3 M
  unsigned long long *kmin;            // M
  unsigned long long *ctr;             // kSplitWords
  int64_t M, T;
  __device__ VoxelAcc acc() const { return VoxelAcc{sum, box, mor, kmin}; }
};
struct SplitIn {
  const int32_t *vox;
  const uint8_t *mask;
  const int32_t *key;
  const int64_t *offsets, *members, *n_clusters_dev;
  int64_t n, n_clusters, n_members;
  int max_size, max_extent;
};
struct SplitOut {  // device pointers, every one nullable
  int32_t *parent;
  uint8_t *depth;
  int32_t *size;
  int64_t *root;
  int32_t *box_lo, *box_hi;
  double *centroid;
  uint8_t *mask_or;
  int32_t *key_min;
  int64_t *key_argmin, *offsets, *members;
  int32_t *label;
  fiesta_hip_split_info *info;
  int64_t part_capacity;
  __device__ VoxelStatsOut stats() const { return VoxelStatsOut{box_lo, box_hi, centroid, mask_or, key_min, key_argmin}; }
};

__device__ inline bool split_bad(const SplitWork &w) { return w.ctr[kSplitBad] != 0; }
__device__ inline bool split_oversize(int size, int ex, int ey, int ez, int max_size, int max_extent) {
  return (max_size > 0 && size > max_size) || (max_extent > 0 && max(ex, max(ey, ez)) > max_extent);
}
__device__ inline void split_box_reset(int32_t *box, int64_t p) { VoxelBox::reset(box + 6 * p); }

__global__ __launch_bounds__(kSplitBlock) void k_split_init(SplitWork w, SplitIn in, SplitOut o) {
  const int64_t stride = (int64_t)gridDim.x * kSplitBlock, t = blockIdx.x * (int64_t)kSplitBlock + threadIdx.x;
  for (int64_t j = t; j < w.T; j += stride) w.flags[j] = 0;
  if (o.label)
    for (int64_t i = t; i < in.n; i += stride) o.label[i] = -1;
  if (t < kSplitWords) w.ctr[t] = 0;
}

// ONE thread block's worth of truth: the effective cluster count K = min(n_clusters, *n_clusters_dev), the member range
// [m0, m1) = [offsets[0], offsets[K]).  Only when that range lies inside [0, n_members] are the members themselves read.
__global__ __launch_bounds__(kSplitBlock) void k_split_validate(SplitWork w, SplitIn in) {
  const int64_t stride = (int64_t)gridDim.x * kSplitBlock, t = blockIdx.x * (int64_t)kSplitBlock + threadIdx.x;
  int64_t K = in.n_clusters;
  if (in.n_clusters_dev) K = min(K, max((int64_t)0, *in.n_clusters_dev));
  int64_t m0 = 0, m1 = 0;
  bool bad = false;
  if (K > 0) {
    m0 = in.offsets[0], m1 = in.offsets[K];
    if (m0 < 0 || m1 > in.n_members || m1 < m0) bad = true, m0 = m1 = 0;
  }
  if (t == 0) w.ctr[kSplitM0] = (unsigned long long)m0, w.ctr[kSplitM1] = (unsigned long long)m1, w.ctr[kSplitK] = (unsigned long long)K;
  if (!bad) {
    for (int64_t k = t; k < K; k += stride)
      if (in.offsets[k] > in.offsets[k + 1] || in.offsets[k] < m0 || in.offsets[k + 1] > m1) bad = true;
    for (int64_t j = m0 + t; j < m1; j += stride) {
      const int64_t i = in.members[j];
      if (i < 0 || i >= in.n)
        bad = true;
      else if (!cluster_valid(in.vox[3 * i], in.vox[3 * i + 1], in.vox[3 * i + 2]))
        bad = true;
    }
  }
  if (bad) atomicOr(&w.ctr[kSplitBad], 1ull);
}

// a head flag at the first member of every non-empty cluster segment; the cluster's index waits there in mid[]
__global__ __launch_bounds__(kSplitBlock) void k_split_seed(SplitWork w, SplitIn in) {
  if (split_bad(w)) return;
  const int64_t stride = (int64_t)gridDim.x * kSplitBlock, K = (int64_t)w.ctr[kSplitK];
  for (int64_t k = blockIdx.x * (int64_t)kSplitBlock + threadIdx.x; k < K; k += stride) {
    const int64_t a = in.offsets[k];
    if (in.offsets[k + 1] > a) w.flags[a] = 2, w.mid[a] = (int)k;
  }
}

// LEVEL < 0: the seed's flags as they stand.  Otherwise the flags of level LEVEL are made here: bit 0 for a member on the high side
// of its part's cut, bit 1 for the first member of a part that is cut.  One work-group per tile; partial[tile] = the tile's sum.
__global__ __launch_bounds__(kSplitBlock) void k_split_partial(SplitWork w, SplitIn in, int level) {
  __shared__ unsigned long long s_wave[kSplitBlock / 64];
  if (split_bad(w) || (level >= 0 && w.ctr[kSplitCuts + level] == 0)) return;
  const int64_t m0 = (int64_t)w.ctr[kSplitM0], m1 = (int64_t)w.ctr[kSplitM1];
  const int cur = level < 0 ? 0 : (int)w.ctr[kSplitCur + level];
  unsigned long long v = 0;
  // (lane t takes positions base + t, base + t + 256, ..: coalesced; a sum does not care which lane holds what)
  for (int k = 0; k < kSplitItems; ++k) {
    const int64_t j = blockIdx.x * (int64_t)kSplitTile + k * kSplitBlock + threadIdx.x;
    int f = 0;
    if (level < 0) {
      f = w.flags[j];
    } else {
      if (j >= m0 && j < m1) {
        const int p = w.part[cur][j], a = w.axis[p];
        if (a >= 0) {
          if (j == w.start[cur][p]) f |= 2;
          if (in.vox[3 * (int64_t)w.mem[cur][j] + a] > w.mid[p]) f |= 1;
        }
      }
      w.flags[j] = (uint8_t)f;
    }
    v += ((unsigned long long)(f >> 1) << 32) | (unsigned long long)(f & 1);
  }
  unsigned long long total;
  (void)block_inclusive<kSplitBlock / 64>(v, 0ull, WaveSum{}, s_wave, &total);
  if (threadIdx.x == 0) w.partial[blockIdx.x] = total;
}

// ONE work-group: the exclusive scan of the n_tiles <= items * 1024 partials in place; the state of the next level
__global__ __launch_bounds__(kSplitScanBlock) void k_split_scan(SplitWork w, int level, int n_tiles, int items) {
  __shared__ unsigned long long s_wave[kSplitScanBlock / 64];
  if (split_bad(w)) return;
  if (level >= 0 && w.ctr[kSplitCuts + level] == 0) {  // nothing was cut at this level: the next one starts from the same state
    if (threadIdx.x == 0) w.ctr[kSplitCur + level + 1] = w.ctr[kSplitCur + level], w.ctr[kSplitParts + level + 1] = w.ctr[kSplitParts + level];
    return;
  }
  const int i0 = threadIdx.x * items;
  unsigned long long v = 0;
  for (int k = 0; k < items; ++k)
    if (i0 + k < n_tiles) v += w.partial[i0 + k];
  unsigned long long total;
  unsigned long long run = block_inclusive<kSplitScanBlock / 64>(v, 0ull, WaveSum{}, s_wave, &total) - v;
  for (int k = 0; k < items; ++k)
    if (i0 + k < n_tiles) {
      const unsigned long long x = w.partial[i0 + k];
      w.partial[i0 + k] = run;
      run += x;
    }
  if (threadIdx.x == 0) {
    const unsigned long long heads = total >> 32;
    if (level < 0) {
      w.ctr[kSplitCur] = 0, w.ctr[kSplitParts] = heads;
      w.start[0][heads] = (int)w.ctr[kSplitM1];
    } else {
      const int nx = (int)w.ctr[kSplitCur + level] ^ 1;
      const unsigned long long P = w.ctr[kSplitParts + level] + heads;
      w.ctr[kSplitCur + level + 1] = (unsigned long long)nx, w.ctr[kSplitParts + level + 1] = P;
      w.start[nx][P] = (int)w.ctr[kSplitM1];
    }
  }
}

// pre[j] = the exclusive scan of the flags at position j: lane t owns kSplitItems consecutive positions
__global__ __launch_bounds__(kSplitBlock) void k_split_rescan(SplitWork w, int level) {
  __shared__ unsigned long long s_wave[kSplitBlock / 64];
  if (split_bad(w) || (level >= 0 && w.ctr[kSplitCuts + level] == 0)) return;
  const int64_t j0 = blockIdx.x * (int64_t)kSplitTile + (int64_t)threadIdx.x * kSplitItems;
  const unsigned long long f8 = *(const unsigned long long *)(w.flags + j0);  // (8-byte aligned: j0 is a multiple of 8)
  unsigned long long v = 0;
#pragma unroll
  for (int k = 0; k < kSplitItems; ++k) {
    const unsigned f = (unsigned)(f8 >> (8 * k)) & 0xFFu;
    v += ((unsigned long long)(f >> 1) << 32) | (unsigned long long)(f & 1u);
  }
  unsigned long long total;
  unsigned long long run = w.partial[blockIdx.x] + block_inclusive<kSplitBlock / 64>(v, 0ull, WaveSum{}, s_wave, &total) - v;
#pragma unroll
  for (int k = 0; k < kSplitItems; ++k) {
    const unsigned f = (unsigned)(f8 >> (8 * k)) & 0xFFu;
    w.pre[j0 + k] = run;
    run += ((unsigned long long)(f >> 1) << 32) | (unsigned long long)(f & 1u);
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) w.pre[w.T] = w.partial[blockIdx.x] + total;
}

// the depth-0 parts: part = the number of heads up to and including the position, minus one
__global__ __launch_bounds__(kSplitBlock) void k_split_first(SplitWork w, SplitIn in) {
  if (split_bad(w)) return;
  const int64_t stride = (int64_t)gridDim.x * kSplitBlock, m0 = (int64_t)w.ctr[kSplitM0], m1 = (int64_t)w.ctr[kSplitM1];
  for (int64_t j = m0 + blockIdx.x * (int64_t)kSplitBlock + threadIdx.x; j < m1; j += stride) {
    const int head = w.flags[j] >> 1, p = (int)(w.pre[j] >> 32) + head - 1;
    w.mem[0][j] = (int)in.members[j];
    w.part[0][j] = p;
    if (head) {
      w.start[0][p] = (int)j, w.par[0][p] = w.mid[j], w.dep[0][p] = 0;
      split_box_reset(w.box, p);
    }
  }
}

// The boxes of the parts at depth `level` (the only ones that can still be oversize).  A wave takes kSplitBoxRun consecutive chunks
// of 64 members.  Per chunk: loop over the DISTINCT parts present (the trip count is uniform across the lanes); the lanes of that
// part reduce among themselves with a butterfly in which the others carry the identity, so every lane holds the part's box of the
// chunk.  The members of a part are contiguous, so the parts of a run come in order: the wave keeps ONE running box, in every lane
// alike, and flushes it when the part changes and at the end of the run -- one flush per wave, run and part.
__device__ inline void split_box_flush(int32_t *box, int c, const VoxelBox &v) {
  // A word only ever moves outwards during this kernel, so a value read now (a relaxed atomic load: the L2's copy, or an older
  // one) that already covers the wave's needs no atomic: after the first waves of a large part almost none does.
  int32_t *b = box + 6 * (int64_t)c;
  if (v.lx < cluster_load(b)) atomicMin(b, v.lx);
  if (v.ly < cluster_load(b + 1)) atomicMin(b + 1, v.ly);
  if (v.lz < cluster_load(b + 2)) atomicMin(b + 2, v.lz);
  if (v.hx > cluster_load(b + 3)) atomicMax(b + 3, v.hx);
  if (v.hy > cluster_load(b + 4)) atomicMax(b + 4, v.hy);
  if (v.hz > cluster_load(b + 5)) atomicMax(b + 5, v.hz);
}
__global__ __launch_bounds__(kSplitBlock) void k_split_box(SplitWork w, SplitIn in, int level) {
  if (split_bad(w) || (level > 0 && w.ctr[kSplitCuts + level - 1] == 0)) return;
  const int64_t m0 = (int64_t)w.ctr[kSplitM0], m1 = (int64_t)w.ctr[kSplitM1];
  const int64_t span = 64 * (int64_t)kSplitBoxRun, stride = (int64_t)gridDim.x * (kSplitBlock / 64) * span;
  const int cur = (int)w.ctr[kSplitCur + level], lane = threadIdx.x & 63;
  for (int64_t run = m0 + (blockIdx.x * (int64_t)(kSplitBlock / 64) + (threadIdx.x >> 6)) * span; run < m1; run += stride) {  // (whole waves: the ballot)
    int rc = -1;  // the running box and its part: uniform
    VoxelBox rb = VoxelBox::identity();
    for (int k = 0; k < kSplitBoxRun; ++k) {
      const int64_t j = run + 64 * (int64_t)k + lane;
      int p = -1, x = 0, y = 0, z = 0;
      bool on = false;
      if (j < m1) {
        p = w.part[cur][j];
        on = w.dep[cur][p] == level;
        if (on) {
          const int64_t i = w.mem[cur][j];
          x = in.vox[3 * i], y = in.vox[3 * i + 1], z = in.vox[3 * i + 2];
        }
      }
      wave_for_each_key(on, p, [&](int c, bool mine, unsigned long long) {
        VoxelBox b = VoxelBox::at(mine, x, y, z);
        b.reduce();
        if (c != rc) {  // (uniform)
          if (rc >= 0 && lane == 0) split_box_flush(w.box, rc, rb);
          rc = c, rb = b;
        } else {
          rb.combine(b);
        }
      });
    }
    if (rc >= 0 && lane == 0) split_box_flush(w.box, rc, rb);
  }
}

// a lane per part: the cut of this level, or none
__global__ __launch_bounds__(kSplitBlock) void k_split_decide(SplitWork w, SplitIn in, int level) {
  if (split_bad(w) || (level > 0 && w.ctr[kSplitCuts + level - 1] == 0)) return;
  const int64_t stride = (int64_t)gridDim.x * kSplitBlock, P = (int64_t)w.ctr[kSplitParts + level];
  const int cur = (int)w.ctr[kSplitCur + level];
  for (int64_t base = blockIdx.x * (int64_t)kSplitBlock + (threadIdx.x & ~63); base < P; base += stride) {
    const int64_t p = base + (threadIdx.x & 63);
    bool cut = false;
    if (p < P) {
      int a = -1;
      if (w.dep[cur][p] == level) {
        const int32_t *b = w.box + 6 * p;
        const int ex = b[3] - b[0] + 1, ey = b[4] - b[1] + 1, ez = b[5] - b[2] + 1;
        // (extent 1 on every axis: members of one voxel, listed more than once -- nothing to cut)
        if (max(ex, max(ey, ez)) >= 2 && split_oversize(w.start[cur][p + 1] - w.start[cur][p], ex, ey, ez, in.max_size, in.max_extent)) {
          a = ex >= ey && ex >= ez ? 0 : ey >= ez ? 1 : 2;
          w.mid[p] = b[a] + ((b[3 + a] - b[a]) >> 1);
          cut = true;
        }
      }
      w.axis[p] = a;
    }
    const unsigned long long b = __ballot(cut);
    if (b && (threadIdx.x & 63) == 0) atomicAdd(&w.ctr[kSplitCuts + level], (unsigned long long)__popcll(b));
  }
}

// the stable partition of every cut part, inside its own range, into the other buffer set; the new part records
__global__ __launch_bounds__(kSplitBlock) void k_split_scatter(SplitWork w, int level) {
  if (split_bad(w) || w.ctr[kSplitCuts + level] == 0) return;
  const int64_t stride = (int64_t)gridDim.x * kSplitBlock, m0 = (int64_t)w.ctr[kSplitM0], m1 = (int64_t)w.ctr[kSplitM1];
  const int cur = (int)w.ctr[kSplitCur + level], nx = cur ^ 1;
  for (int64_t j = m0 + blockIdx.x * (int64_t)kSplitBlock + threadIdx.x; j < m1; j += stride) {
    const int p = w.part[cur][j], s = w.start[cur][p], a = w.axis[p];
    const unsigned long long ps = w.pre[s];
    int q = p + (int)(ps >> 32);  // (the cut parts before this one: each of them made one more part)
    int64_t at = j;
    int n_low = 0;
    if (a >= 0) {
      const int e = w.start[cur][p + 1];
      const int n_high = (int)(uint32_t)w.pre[e] - (int)(uint32_t)ps, r_high = (int)(uint32_t)w.pre[j] - (int)(uint32_t)ps;
      n_low = e - s - n_high;
      if (w.flags[j] & 1)
        at = (int64_t)s + n_low + r_high, ++q;
      else
        at = j - r_high;
    }
    w.mem[nx][at] = w.mem[cur][j];
    w.part[nx][at] = q;
    if (j == s) {  // the part's first member writes the records (it may itself go to the high side: q0 is the low child's index)
      const int q0 = p + (int)(ps >> 32);
      w.start[nx][q0] = s, w.par[nx][q0] = w.par[cur][p];
      if (a < 0) {
        w.dep[nx][q0] = w.dep[cur][p];
      } else {
        w.dep[nx][q0] = w.dep[nx][q0 + 1] = level + 1;
        w.start[nx][q0 + 1] = s + n_low, w.par[nx][q0 + 1] = w.par[cur][p];
        split_box_reset(w.box, q0), split_box_reset(w.box, q0 + 1);
      }
    }
  }
}

__global__ __launch_bounds__(kSplitBlock) void k_split_acc_init(SplitWork w, int levels) {
  if (split_bad(w)) return;
  const int64_t stride = (int64_t)gridDim.x * kSplitBlock, P = (int64_t)w.ctr[kSplitParts + levels];
  for (int64_t p = blockIdx.x * (int64_t)kSplitBlock + threadIdx.x; p < P; p += stride) {
    w.acc().reset(p), w.proot[p] = INT32_MAX;
  }
}

// labels, the output members and the per-part reductions: the wave aggregation of wave_ops.hpp (VoxelStats)
__global__ __launch_bounds__(kSplitBlock) void k_split_stats(SplitWork w, SplitIn in, SplitOut o, int levels) {
  if (split_bad(w)) return;
  const int64_t stride = (int64_t)gridDim.x * kSplitBlock, m0 = (int64_t)w.ctr[kSplitM0], m1 = (int64_t)w.ctr[kSplitM1];
  const int cur = (int)w.ctr[kSplitCur + levels], lane = threadIdx.x & 63;
  for (int64_t base = m0 + blockIdx.x * (int64_t)kSplitBlock + (threadIdx.x & ~63); base < m1; base += stride) {
    const int64_t j = base + lane;
    const bool on = j < m1;
    int p = -1, i = INT32_MAX, x = 0, y = 0, z = 0;
    uint32_t mk = 0;
    unsigned long long kp = ~0ull;
    if (on) {
      p = w.part[cur][j], i = w.mem[cur][j];
      if (o.members) o.members[j] = i;
      if (o.label) atomicMax(&o.label[i], p);
      x = in.vox[3 * (int64_t)i], y = in.vox[3 * (int64_t)i + 1], z = in.vox[3 * (int64_t)i + 2];
      if (in.mask) mk = in.mask[i];
      if (in.key) {
        const int kv = in.key[i];
        if (kv >= 0) kp = ((unsigned long long)(uint32_t)kv << 32) | (unsigned long long)(uint32_t)i;
      }
    }
    wave_for_each_key(on, p, [&](int c, bool mine, unsigned long long same) {
      VoxelStats st = VoxelStats::at(mine, x, y, z, mk, kp);
      int ri = mine ? i : INT32_MAX;  // the part's root: its lowest entry index
      if (__popcll(same) > 1) st.reduce(), ri = wave_min(ri);
      if (wave_first_of(same)) st.commit(w.acc(), c), atomicMin(&w.proot[c], ri);
    });
  }
}

// per part (and the closing offset): the outputs below part_capacity, the centroid in k_cluster_finish's operation order (no
// contraction: -ffp-contract=off); the totals over ALL parts, reduced in the wave first
__global__ __launch_bounds__(kSplitBlock) void k_split_finish(SplitWork w, SplitIn in, SplitOut o, int levels, double res, double ox, double oy, double oz) {
  if (split_bad(w)) return;
  const int64_t stride = (int64_t)gridDim.x * kSplitBlock, P = (int64_t)w.ctr[kSplitParts + levels];
  const int cur = (int)w.ctr[kSplitCur + levels];
  for (int64_t base = blockIdx.x * (int64_t)kSplitBlock + (threadIdx.x & ~63); base <= P; base += stride) {
    const int64_t p = base + (threadIdx.x & 63);
    int size = 0, deep = 0, over = 0, cutc = 0;
    if (p == P && o.offsets && p <= o.part_capacity) o.offsets[p] = (int64_t)w.ctr[kSplitM1];
    if (p < P) {
      const int32_t *b = w.box + 6 * p;
      const int s = w.start[cur][p];
      size = w.start[cur][p + 1] - s, deep = w.dep[cur][p];
      over = split_oversize(size, b[3] - b[0] + 1, b[4] - b[1] + 1, b[5] - b[2] + 1, in.max_size, in.max_extent);
      cutc = deep > 0 && (p == 0 || w.par[cur][p - 1] != w.par[cur][p]);
      if (o.offsets && p <= o.part_capacity) o.offsets[p] = s;
      if (p < o.part_capacity) {
        if (o.parent) o.parent[p] = w.par[cur][p];
        if (o.depth) o.depth[p] = (uint8_t)deep;
        if (o.size) o.size[p] = size;
        if (o.root) o.root[p] = w.proot[p];
        voxel_stats_write(w.acc(), o.stats(), p, size, res, ox, oy, oz);
      }
    }
    size = wave_max(size), deep = wave_max(deep), over = wave_sum(over), cutc = wave_sum(cutc);
    if ((threadIdx.x & 63) == 0) {
      if (size) atomicMax(&w.ctr[kSplitLargest], (unsigned long long)size);
      if (deep) atomicMax(&w.ctr[kSplitDeepest], (unsigned long long)deep);
      if (over) atomicAdd(&w.ctr[kSplitOver], (unsigned long long)over);
      if (cutc) atomicAdd(&w.ctr[kSplitCutClusters], (unsigned long long)cutc);
    }
  }
}

__global__ void k_split_info(SplitWork w, SplitOut o, int levels) {
  if (threadIdx.x != 0 || blockIdx.x != 0 || !o.info) return;
  fiesta_hip_split_info f{};
  if (split_bad(w)) {
    f.status = FIESTA_HIP_SPLIT_INVALID;
  } else {
    f.n_parts = (int64_t)w.ctr[kSplitParts + levels], f.n_members = (int64_t)w.ctr[kSplitM1];
    f.n_split_clusters = (int64_t)w.ctr[kSplitCutClusters], f.n_oversize = (int64_t)w.ctr[kSplitOver];
    f.largest = (int64_t)w.ctr[kSplitLargest], f.depth = (int64_t)w.ctr[kSplitDeepest], f.status = FIESTA_HIP_SPLIT_OK;
  }
  *o.info = f;
}

// enqueue the passes; every pointer of `in` and `o` is a device pointer
inline void split_enqueue(hipStream_t st, SplitScratch &S, const SplitIn &in, const SplitOut &o, int max_depth, double res, const double *org) {
  const int64_t M = std::max<int64_t>(in.n_members, 1), tiles = (M + kSplitTile - 1) / kSplitTile, T = tiles * kSplitTile;
  S.i32.ensure((size_t)(20 * M + 2), st), S.u64.ensure((size_t)(T + 1 + tiles + 1 + 4 * M + kSplitWords), st), S.u8.ensure((size_t)T, st);
  SplitWork w{};
  int32_t *a = S.i32.p;
  const auto take = [&](int64_t count) { int32_t *q = a; a += count; return q; };
  w.mem[0] = take(M), w.mem[1] = take(M), w.part[0] = take(M), w.part[1] = take(M), w.start[0] = take(M + 1), w.start[1] = take(M + 1);
  w.par[0] = take(M), w.par[1] = take(M), w.dep[0] = take(M), w.dep[1] = take(M), w.box = take(6 * M), w.axis = take(M), w.mid = take(M);
  w.proot = take(M), w.mor = (uint32_t *)take(M);
  w.pre = S.u64.p, w.partial = w.pre + T + 1, w.sum = w.partial + tiles + 1, w.kmin = w.sum + 3 * M, w.ctr = w.kmin + M;
  w.flags = S.u8.p, w.M = M, w.T = T;
  const auto blocks = [](int64_t items) { return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((items + kSplitBlock - 1) / kSplitBlock, kClusterMaxBlocks))); };
  const dim3 B(kSplitBlock), per_member = blocks(M), per_tile((unsigned)tiles);
  const int items = (int)((tiles + kSplitScanBlock - 1) / kSplitScanBlock);
  const int levels = in.max_size > 0 || in.max_extent > 0 ? max_depth : 0;
  hipLaunchKernelGGL(k_split_init, blocks(std::max(T, in.n)), B, 0, st, w, in, o);
  hipLaunchKernelGGL(k_split_validate, blocks(std::max(M, in.n_clusters)), B, 0, st, w, in);
  hipLaunchKernelGGL(k_split_seed, blocks(in.n_clusters), B, 0, st, w, in);
  hipLaunchKernelGGL(k_split_partial, per_tile, B, 0, st, w, in, -1);
  hipLaunchKernelGGL(k_split_scan, dim3(1), dim3(kSplitScanBlock), 0, st, w, -1, (int)tiles, items);
  hipLaunchKernelGGL(k_split_rescan, per_tile, B, 0, st, w, -1);
  hipLaunchKernelGGL(k_split_first, per_member, B, 0, st, w, in);
  for (int level = 0; level < levels; ++level) {
    hipLaunchKernelGGL(k_split_box, blocks((M + kSplitBoxRun - 1) / kSplitBoxRun), B, 0, st, w, in, level);
    hipLaunchKernelGGL(k_split_decide, per_member, B, 0, st, w, in, level);
    hipLaunchKernelGGL(k_split_partial, per_tile, B, 0, st, w, in, level);
    hipLaunchKernelGGL(k_split_scan, dim3(1), dim3(kSplitScanBlock), 0, st, w, level, (int)tiles, items);
    hipLaunchKernelGGL(k_split_rescan, per_tile, B, 0, st, w, level);
    hipLaunchKernelGGL(k_split_scatter, per_member, B, 0, st, w, level);
  }
  hipLaunchKernelGGL(k_split_acc_init, per_member, B, 0, st, w, levels);
  hipLaunchKernelGGL(k_split_stats, per_member, B, 0, st, w, in, o, levels);
  hipLaunchKernelGGL(k_split_finish, per_member, B, 0, st, w, in, o, levels, res, org[0], org[1], org[2]);
  hipLaunchKernelGGL(k_split_info, dim3(1), dim3(64), 0, st, w, o, levels);
  FIESTA_HIP_CHECK(hipGetLastError());
}

// Both variants of the call on a map's stream; res / org: the map's resolution and origin -- nothing else of a map is read, so
// both stores share this function.  The device variant only enqueues.  The host variant (its data errors were refused by the
// caller) stages the inputs through P.in and every output through P.out, runs, copies everything back and synchronises once.
inline void split_clusters_run(hipStream_t st, PlannerScratch &P, double res, const double *org, const SplitArgs &a) {
  const fiesta_hip_split_result none{};
  const fiesta_hip_split_result &r = a.res ? *a.res : none;
  if (a.dev) {
    const SplitIn si{a.vox, a.mask, a.key, a.offsets, a.members, a.n_clusters_dev, a.n, a.n_clusters, a.n_members, a.max_size, a.max_extent};
    const SplitOut so{r.parent, r.depth, r.size, r.root, r.box_lo, r.box_hi, r.centroid, r.mask_or, r.key_min, r.key_argmin, r.offsets, r.members, r.label,
                      a.info, a.part_capacity};
    split_enqueue(st, P.split, si, so, a.max_depth, res, org);
    return;
  }
  const size_t n = (size_t)a.n, K = (size_t)a.n_clusters, M = (size_t)a.n_members, C = (size_t)std::min<int64_t>(a.n_members, a.part_capacity);
  Staging in{P.in, st}, out{P.out, st};
  const auto offsets_in = in.add(a.offsets, K ? K + 1 : 0), members_in = in.add(a.members, M);
  const auto vox = in.add(a.vox, 3 * n), key = in.add(a.key, n);
  const auto mask = in.add(a.mask, n);
  in.alloc(), in.up(offsets_in, K ? K + 1 : 0), in.up(members_in, M), in.up(vox, 3 * n), in.up(key, n), in.up(mask, n);
  const SplitIn si{in.dev(vox), in.dev(mask), in.dev(key), in.dev(offsets_in), in.dev(members_in), nullptr, a.n, a.n_clusters, a.n_members, a.max_size, a.max_extent};
  const auto info = out.add(a.info, 1);
  const auto root = out.add(r.root, C), key_argmin = out.add(r.key_argmin, C), offsets = out.add(r.offsets, C + 1), members = out.add(r.members, M);
  const auto centroid = out.add(r.centroid, 3 * C);
  const auto parent = out.add(r.parent, C), size = out.add(r.size, C), box_lo = out.add(r.box_lo, 3 * C), box_hi = out.add(r.box_hi, 3 * C),
             key_min = out.add(r.key_min, C), label = out.add(r.label, n);
  const auto depth = out.add(r.depth, C), mask_or = out.add(r.mask_or, C);
  out.alloc();
  const SplitOut so{out.dev(parent),  out.dev(depth),      out.dev(size),    out.dev(root),    out.dev(box_lo), out.dev(box_hi), out.dev(centroid), out.dev(mask_or),
                    out.dev(key_min), out.dev(key_argmin), out.dev(offsets), out.dev(members), out.dev(label),  out.dev(info),   (int64_t)C};
  // (what the call does not write reads 0; the member positions below offsets[0] belong to no part and keep the input's value)
  FIESTA_HIP_CHECK(hipMemsetAsync(P.out.p, 0, out.end, st));
  if (r.members && M) FIESTA_HIP_CHECK(hipMemcpyAsync(out.dev(members), in.dev(members_in), M * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
  split_enqueue(st, P.split, si, so, a.max_depth, res, org);
  out.back(info, 1), out.back(label, n), out.back(members, M);
  out.back(parent, C), out.back(depth, C), out.back(size, C), out.back(root, C), out.back(box_lo, 3 * C), out.back(box_hi, 3 * C), out.back(centroid, 3 * C);
  out.back(mask_or, C), out.back(key_min, C), out.back(key_argmin, C), out.back(offsets, C + 1);
  FIESTA_HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace
}  // namespace fiesta
