// fiesta_amd/csrc/cluster_kernels.hpp -- connected clusters of a sparse voxel list: fiesta_hip_cluster_voxels / _dev (include/fiesta_hip.h).
//
// The step between fiesta_hip_get_frontier_voxels and fiesta_hip_reach_field: a planner visits FRONTIERS, the connected groups of
// frontier voxels.  The call reads nothing of a map but its resolution and origin; everything is integer arithmetic but the
// centroids (one f64 expression per coordinate, the operation order of reach_path_store).  Passes, all on the map's stream, none
// cooperative, no work-group ever waits for another:
//   k_cluster_init     table slots empty, per-entry counters 0, per-cluster accumulators at their identities, the counters 0
//   k_cluster_insert   one open-addressing table of packed 64-bit voxel keys (linear probing from a mixed hash): a 64-bit atomicCAS
//                      claims the key, an atomicMin on the slot's entry index leaves the voxel's REPRESENTATIVE (lowest entry) there
//   k_cluster_seed     parent[i] = i for a representative (its own union-find tree), its representative for a later duplicate
//   k_cluster_link<C>  per representative the lexicographically FORWARD half of the stencil (3 / 9 / 13 probes): a neighbour found in
//                      the table joins the two trees of a lock-free union-find over entry indices (see cluster_unite)
//   k_cluster_flatten  every entry finds its root; representatives add to their root's counter, one atomic per wave and root
//   k_cluster_number   ONE work-group striding with a carry (block_scan_stride of wave_ops.hpp, 4096 entries per trip): roots with
//                      size >= min_size get ids in increasing root order, their sizes scan into the member offsets; the totals
//   k_cluster_reduce   labels; per-cluster coordinate sums, box, mask OR, packed (key, index) minimum and the member scatter, all
//                      aggregated inside the wave first: one atomic per wave, cluster and quantity (see there)
//   k_cluster_finish   per written cluster: box, centroid, mask_or, key_min / key_argmin out of the accumulators
// Every quantity is a commutative exact integer reduction, roots are the lowest entry index of their component (hooks go from the
// higher root to the lower), ids follow root order: all outputs but the order inside a member segment are the same bits for any
// launch shape, scheduling and table size, and the bits of fiesta_amd.cluster_model.  No LDS outside the numbering pass, no scratch.
#pragma once
#include <algorithm>
#include <climits>

#include "../../include/fiesta_hip.h"
#include "common.hpp"
#include "planner.hpp"
#include "planner_args.hpp"
#include "wave_ops.hpp"

namespace fiesta {
namespace {  // (planner.hip alone includes this header; the namespace is part of the kernels' symbol names)

constexpr int64_t kClusterMaxEntries = 1ll << 24;
constexpr int kClusterCoordLimit = (1 << 20) - 1;  // |c| >= this: INVALID (c and c +- 1, biased by 2^20, fit 21 bits)
constexpr unsigned long long kClusterEmpty = ~0ull;  // (a valid key has bit 63 clear)
constexpr int kClusterDup = 1 << 30;                 // lab[i]: root | kClusterDup for a later duplicate, -1 for an invalid entry
constexpr int kClusterBlock = 256, kClusterMaxBlocks = 4096;
constexpr int kClusterScanBlock = 1024, kClusterScanItems = 4;

// device view of the map's ClusterScratch for one call.  S: table slots (a power of two >= 2 n); C: clusters that get accumulators
struct ClusterWork {
  unsigned long long *keys;  // S
  int32_t *tidx;             // S: lowest entry index that named the slot's voxel
  int32_t *lab;              // n: insert .. link: the entry's slot (-1: invalid); from flatten on: root | dup bit (-1: invalid)
  int32_t *parent;           // n: union-find; from number on, at a kept root: the member cursor of its cluster
  int32_t *cnt;              // n: at a root: its size; from number on: its cluster id (-1: dropped)
  unsigned long long *sum;   // 3 C: exact coordinate sums (two's complement)
  int32_t *box;              // 6 C: min x, y, z, max x, y, z
  uint32_t *mor;             // C
  unsigned long long *kmin;  // C: (key << 32) | entry index, over representatives with key >= 0
  int32_t *csize;            // C
  unsigned long long *ctr;   // [0] invalid entries, [1] duplicates
  int64_t S, C;
  __device__ VoxelAcc acc() const { return VoxelAcc{sum, box, mor, kmin}; }
};
struct ClusterIn {
  const int32_t *vox;
  const uint8_t *mask;
  const int32_t *key;
  const unsigned long long *n_dev;  // nullable
  int64_t n;
};
struct ClusterOut {  // device pointers, every one nullable
  int32_t *label, *size;
  int64_t *root;
  int32_t *box_lo, *box_hi;
  double *centroid;
  uint8_t *mask_or;
  int32_t *key_min;
  int64_t *key_argmin, *offsets, *members;
  fiesta_hip_cluster_info *info;
  int64_t cluster_capacity, member_capacity;
  __device__ VoxelStatsOut stats() const { return VoxelStatsOut{box_lo, box_hi, centroid, mask_or, key_min, key_argmin}; }
};

__device__ inline int64_t cluster_count(const ClusterIn &in) {
  if (!in.n_dev) return in.n;
  const unsigned long long d = *in.n_dev;
  return d < (unsigned long long)in.n ? (int64_t)d : in.n;
}
__device__ inline bool cluster_valid(int x, int y, int z) {
  return x > -kClusterCoordLimit && x < kClusterCoordLimit && y > -kClusterCoordLimit && y < kClusterCoordLimit && z > -kClusterCoordLimit &&
         z < kClusterCoordLimit;
}
__device__ inline unsigned long long cluster_pack(int x, int y, int z) {
  return ((unsigned long long)(x + (1 << 20)) << 42) | ((unsigned long long)(y + (1 << 20)) << 21) | (unsigned long long)(z + (1 << 20));
}
// a mixing hash (the splitmix64 finaliser): lattice coordinates and keys that differ in high bits only spread over the table
__device__ inline uint64_t cluster_hash(unsigned long long k) {
  k ^= k >> 30, k *= 0xBF58476D1CE4E5B9ull;
  k ^= k >> 27, k *= 0x94D049BB133111EBull;
  return k ^ (k >> 31);
}
__device__ inline int cluster_load(const int32_t *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

__global__ __launch_bounds__(kClusterBlock) void k_cluster_init(ClusterWork w, ClusterIn in) {
  const int64_t n = cluster_count(in), stride = (int64_t)gridDim.x * kClusterBlock;
  const int64_t t = blockIdx.x * (int64_t)kClusterBlock + threadIdx.x;
  for (int64_t s = t; s < w.S; s += stride) w.keys[s] = kClusterEmpty, w.tidx[s] = INT32_MAX;
  for (int64_t i = t; i < n; i += stride) w.cnt[i] = 0;
  for (int64_t k = t; k < w.C; k += stride) w.acc().reset(k), w.csize[k] = 0;
  if (t < 2) w.ctr[t] = 0;
}

// The table holds at most n distinct keys in S >= 2 n slots, so a probe sequence always meets its key or an empty slot.  A slot's key
// is written once (CAS from empty) and never changes: a lane that reads another key moves on, nobody waits.
__global__ __launch_bounds__(kClusterBlock) void k_cluster_insert(ClusterWork w, ClusterIn in) {
  const int64_t n = cluster_count(in), stride = (int64_t)gridDim.x * kClusterBlock;
  const uint64_t m = (uint64_t)w.S - 1;
  for (int64_t base = (blockIdx.x * (int64_t)kClusterBlock + (threadIdx.x & ~63)); base < n; base += stride) {  // (whole waves: the ballot)
    const int64_t i = base + (threadIdx.x & 63);
    bool bad = false;
    if (i < n) {
      const int x = in.vox[3 * i], y = in.vox[3 * i + 1], z = in.vox[3 * i + 2];
      bad = !cluster_valid(x, y, z);
      if (bad) {
        w.lab[i] = -1;
      } else {
        const unsigned long long k = cluster_pack(x, y, z);
        uint64_t s = cluster_hash(k) & m;
        while (true) {
          unsigned long long cur = __atomic_load_n(&w.keys[s], __ATOMIC_RELAXED);
          if (cur == kClusterEmpty) cur = atomicCAS(&w.keys[s], kClusterEmpty, k);
          if (cur == kClusterEmpty || cur == k) break;
          s = (s + 1) & m;
        }
        atomicMin(&w.tidx[s], (int)i);
        w.lab[i] = (int)s;
      }
    }
    const unsigned long long b = __ballot(bad);
    if (b && (threadIdx.x & 63) == 0) atomicAdd(&w.ctr[0], (unsigned long long)__popcll(b));
  }
}

__global__ __launch_bounds__(kClusterBlock) void k_cluster_seed(ClusterWork w, ClusterIn in) {
  const int64_t n = cluster_count(in), stride = (int64_t)gridDim.x * kClusterBlock;
  for (int64_t base = (blockIdx.x * (int64_t)kClusterBlock + (threadIdx.x & ~63)); base < n; base += stride) {
    const int64_t i = base + (threadIdx.x & 63);
    bool dup = false;
    if (i < n) {
      const int s = w.lab[i];
      const int rep = s < 0 ? -1 : w.tidx[s];
      w.parent[i] = rep;
      dup = s >= 0 && rep != (int)i;
    }
    const unsigned long long b = __ballot(dup);
    if (b && (threadIdx.x & 63) == 0) atomicAdd(&w.ctr[1], (unsigned long long)__popcll(b));
  }
}

// The union-find (the ECL-CC scheme: Jaiganesh & Burtscher, HPDC 2018).  parent[] holds entry indices; only representatives are
// linked, a later duplicate is a leaf under its representative.
// INVARIANT  parent[x] <= x, and parent[x] is an ancestor-or-self of x in the forest that the hooks alone define.  Two kinds of
//   store keep it: a HOOK, atomicCAS(&parent[hi], hi, lo) with lo < hi, which succeeds only while hi is a root, and a COMPRESSION
//   store parent[prev] = next, where next was read as the parent of the parent of prev: an ancestor of prev, below it.  A
//   compression store can overwrite a lower ancestor that another lane stored meanwhile; the value is still an ancestor, so the
//   set of nodes a tree holds never shrinks and trees only ever merge.
// TERMINATION  cluster_find follows strictly decreasing indices (it advances only while cur > parent[cur]) and so ends within x
//   steps whatever other lanes do.  In cluster_unite a failed CAS returns the value another lane put into parent[hi]: below hi.
//   Every retry therefore strictly lowers max(a, b), which is bounded below by 0.  No lane waits for another lane's progress: a
//   failed CAS means someone else advanced, and the lane goes on from what it read.
// RESULT  when the kernel has ended, every edge {u, v} had a moment at which one CAS hooked the root of one under a node of the
//   other's tree or found them equal, so the two are in one tree for good; a tree's root is below all its nodes, hence the lowest
//   entry index of its component -- whatever the order of the hooks.
// MEMORY ORDER  every access to parent[] in this kernel is a relaxed atomic (device scope: the L2 is the point of coherence, the
//   loads are not served by a stale per-CU line).  No ordering BETWEEN locations is needed: the argument above only uses that
//   each single location is coherent, that a CAS is atomic, and that values read were stored by someone.  The kernel boundary
//   orders the table (insert, seed) before the links and the links before the flatten pass.
__device__ inline int cluster_find(int32_t *parent, int x) {
  int cur = cluster_load(&parent[x]);
  if (cur != x) {
    int prev = x, next;
    while (cur > (next = cluster_load(&parent[cur]))) {
      __atomic_store_n(&parent[prev], next, __ATOMIC_RELAXED);
      prev = cur;
      cur = next;
    }
  }
  return cur;
}
__device__ inline void cluster_unite(int32_t *parent, int u, int v) {
  int a = cluster_find(parent, u), b = cluster_find(parent, v);
  while (a != b) {
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int old = atomicCAS(&parent[hi], hi, lo);
    if (old == hi) return;  // hooked
    a = old, b = lo;        // hi was no root any more: go on from its parent, which is below hi
  }
}

// forward half of the stencil: (dx, dy, dz) > (0, 0, 0) lexicographically, changing at most 1 / 2 / 3 axes for CONN 6 / 18 / 26
template <int CONN>
__global__ __launch_bounds__(kClusterBlock) void k_cluster_link(ClusterWork w, ClusterIn in) {
  const int64_t n = cluster_count(in), stride = (int64_t)gridDim.x * kClusterBlock;
  const uint64_t m = (uint64_t)w.S - 1;
  for (int64_t i = blockIdx.x * (int64_t)kClusterBlock + threadIdx.x; i < n; i += stride) {
    const int s = w.lab[i];
    if (s < 0 || w.tidx[s] != (int)i) continue;  // invalid, or a later duplicate
    const unsigned long long k = w.keys[s];
#pragma unroll
    for (int d = 14; d < 27; ++d) {
      const int dx = d / 9 - 1, dy = (d / 3) % 3 - 1, dz = d % 3 - 1, ch = (dx != 0) + (dy != 0) + (dz != 0);
      if (ch > (CONN == 6 ? 1 : CONN == 18 ? 2 : 3)) continue;
      // (every field of k lies in [2, 2^21 - 2]: +-1 neither carries nor borrows; a neighbour outside the valid range is never in the table)
      const unsigned long long nk = k + (unsigned long long)(dx * (1ll << 42) + dy * (1ll << 21) + (long long)dz);
      uint64_t t = cluster_hash(nk) & m;
      int j = -1;
      while (true) {
        const unsigned long long cur = w.keys[t];
        if (cur == nk) j = w.tidx[t];
        if (cur == nk || cur == kClusterEmpty) break;
        t = (t + 1) & m;
      }
      if (j >= 0) cluster_unite(w.parent, (int)i, j);
    }
  }
}

// lab[i] = root (| dup bit); cnt[root] += 1 per representative.  Finds still compress (ancestor stores, as above); the answer
// goes to lab[], which only lane i touches.  Lanes of a wave mostly share a root: one atomicAdd per wave and distinct root.
__global__ __launch_bounds__(kClusterBlock) void k_cluster_flatten(ClusterWork w, ClusterIn in) {
  const int64_t n = cluster_count(in), stride = (int64_t)gridDim.x * kClusterBlock;
  const int lane = threadIdx.x & 63;
  for (int64_t base = (blockIdx.x * (int64_t)kClusterBlock + (threadIdx.x & ~63)); base < n; base += stride) {
    const int64_t i = base + lane;
    int root = -1;
    bool rep = false;
    if (i < n) {
      const int s = w.lab[i];
      if (s >= 0) {
        rep = w.tidx[s] == (int)i;
        root = cluster_find(w.parent, (int)i);
        w.lab[i] = rep ? root : (root | kClusterDup);
      }
    }
    wave_count_keys(w.cnt, rep, root);
  }
}

// One work-group, kClusterScanBlock * kClusterScanItems entries per trip, the carry in a register.  Entry i is a root iff
// lab[i] == i.  One 64-bit add scans both quantities: the number of kept roots (high word) and their sizes (low word; both <= 2^24).
__global__ __launch_bounds__(kClusterScanBlock) void k_cluster_number(ClusterWork w, ClusterIn in, ClusterOut o, int min_size) {
  __shared__ unsigned long long s_wave[kClusterScanBlock / 64];
  __shared__ unsigned long long s_dropped;
  __shared__ int s_largest;
  const int64_t n = cluster_count(in);
  const int tid = threadIdx.x;
  if (tid == 0) s_dropped = 0, s_largest = 0;
  unsigned long long dropped = 0;
  int largest = 0;
  const unsigned long long carry = block_scan_stride<kClusterScanItems, kClusterScanBlock / 64>(
      n, s_wave,
      [&](int64_t i) -> unsigned long long {  // a kept root's word; a dropped root is marked here, its word is 0
        if (w.lab[i] != (int)i) return 0;
        const int sz = w.cnt[i];
        if (sz >= min_size) {
          largest = max(largest, sz);
          return (1ull << 32) + (unsigned long long)sz;
        }
        ++dropped, w.cnt[i] = -1;
        return 0;
      },
      [&](int64_t i, unsigned long long run, unsigned long long v) {
        if (!v) return;
        const int64_t id = (int64_t)(run >> 32), at = (int64_t)(run & 0xFFFFFFFFull);
        const int sz = (int)(v & 0xFFFFFFFFull);
        w.cnt[i] = (int)id;
        w.parent[i] = (int)at;
        if (id < w.C) w.csize[id] = sz;
        if (id < o.cluster_capacity) {
          if (o.size) o.size[id] = sz;
          if (o.root) o.root[id] = i;
        }
        if (id <= o.cluster_capacity && o.offsets) o.offsets[id] = at;
      });
  if (dropped) atomicAdd(&s_dropped, dropped);
  if (largest) atomicMax(&s_largest, largest);
  __syncthreads();
  if (tid == 0) {
    const int64_t K = (int64_t)(carry >> 32), members = (int64_t)(carry & 0xFFFFFFFFull);
    if (o.offsets && K <= o.cluster_capacity) o.offsets[K] = members;
    if (o.info) {
      o.info->n_clusters = K, o.info->n_members = members;
      o.info->n_invalid = (int64_t)w.ctr[0], o.info->n_duplicates = (int64_t)w.ctr[1];
      o.info->n_dropped_clusters = (int64_t)s_dropped, o.info->largest = s_largest;
    }
  }
}

// Labels, the per-cluster reductions and the member scatter.  A frontier list comes out of a spatial sweep, so the lanes of a wave
// mostly share a cluster: a cluster of 10^5 voxels must not become 10^5 atomics on one address.  Per wave: loop over the DISTINCT
// clusters present (the first unserved lane's id, a ballot of equality); the lanes of that cluster reduce among themselves with a
// butterfly in which the others carry the identity (a wave's coordinate sum fits 32 bits: 64 * 2^20), and its first lane issues
// ONE atomic per quantity.  A cluster alone in its lane skips the butterfly.  The trip count is the number of distinct clusters
// in the wave, uniform across its lanes.  Only clusters with an id below C have accumulators; members are scattered for every
// kept cluster through the cursor that the numbering pass left at the root.
__global__ __launch_bounds__(kClusterBlock) void k_cluster_reduce(ClusterWork w, ClusterIn in, ClusterOut o) {
  const int64_t n = cluster_count(in), stride = (int64_t)gridDim.x * kClusterBlock;
  const int lane = threadIdx.x & 63;
  for (int64_t base = (blockIdx.x * (int64_t)kClusterBlock + (threadIdx.x & ~63)); base < n; base += stride) {
    const int64_t i = base + lane;
    int id = -1, root = -1, x = 0, y = 0, z = 0;
    uint32_t mk = 0;
    unsigned long long kp = ~0ull;
    bool rep = false;
    if (i < n) {
      const int l = w.lab[i];
      if (l >= 0) {
        root = l & ~kClusterDup;
        id = w.cnt[root];
        rep = !(l & kClusterDup) && id >= 0;
      }
      if (o.label) o.label[i] = id;
      if (rep) {
        x = in.vox[3 * i], y = in.vox[3 * i + 1], z = in.vox[3 * i + 2];
        if (in.mask) mk = in.mask[i];
        if (in.key) {
          const int kv = in.key[i];
          if (kv >= 0) kp = ((unsigned long long)(uint32_t)kv << 32) | (unsigned long long)(uint32_t)i;
        }
      }
    }
    wave_for_each_key(rep, id, [&](int c, bool mine, unsigned long long same) {
      const int cnt = __popcll(same), first = __ffsll((long long)same) - 1;
      // members: the first lane takes cnt places at the cluster's cursor, lane r-th of the cluster writes the r-th of them
      int at = 0;
      if (lane == first) at = atomicAdd(&w.parent[root], cnt);
      at = __shfl(at, first) + __popcll(same & ((1ull << lane) - 1));
      if (mine && o.members && at < o.member_capacity) o.members[at] = i;
      if (c >= w.C) return;  // (uniform)
      VoxelStats st = VoxelStats::at(mine, x, y, z, mk, kp);
      if (cnt > 1) st.reduce();
      if (lane == first) st.commit(w.acc(), c);
    });
  }
}

// per cluster below min(K, C); the centroid in the operation order of reach_path_store (no contraction: -ffp-contract=off)
__global__ __launch_bounds__(kClusterBlock) void k_cluster_finish(ClusterWork w, ClusterOut o, double res, double ox, double oy, double oz) {
  const int64_t stride = (int64_t)gridDim.x * kClusterBlock;
  for (int64_t k = blockIdx.x * (int64_t)kClusterBlock + threadIdx.x; k < w.C; k += stride) {
    const int size = w.csize[k];
    if (size <= 0) continue;  // beyond the number of clusters
    voxel_stats_write(w.acc(), o.stats(), k, size, res, ox, oy, oz);
  }
}

// enqueue the passes; every pointer of `in` and `o` is a device pointer
inline void cluster_enqueue(hipStream_t st, ClusterScratch &S, const ClusterIn &in, const ClusterOut &o, int connectivity, int min_size, double res,
                            const double *org) {
  const int64_t n = in.n;
  int64_t slots = 64;
  while (slots < 2 * n) slots *= 2;
  const int64_t C = std::min<int64_t>(n, o.cluster_capacity);
  S.keys.ensure((size_t)slots, st), S.tidx.ensure((size_t)slots, st);
  S.lab.ensure((size_t)std::max<int64_t>(n, 1), st), S.parent.ensure((size_t)std::max<int64_t>(n, 1), st), S.cnt.ensure((size_t)std::max<int64_t>(n, 1), st);
  S.sum.ensure((size_t)std::max<int64_t>(3 * C, 1), st), S.box.ensure((size_t)std::max<int64_t>(6 * C, 1), st);
  S.mor.ensure((size_t)std::max<int64_t>(C, 1), st), S.kmin.ensure((size_t)std::max<int64_t>(C, 1), st), S.csize.ensure((size_t)std::max<int64_t>(C, 1), st);
  S.ctr.ensure(2, st);
  const ClusterWork w{S.keys.p, S.tidx.p, S.lab.p, S.parent.p, S.cnt.p, S.sum.p, S.box.p, S.mor.p, S.kmin.p, S.csize.p, S.ctr.p, slots, C};
  const auto blocks = [](int64_t items) { return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((items + kClusterBlock - 1) / kClusterBlock, kClusterMaxBlocks))); };
  hipLaunchKernelGGL(k_cluster_init, blocks(slots), dim3(kClusterBlock), 0, st, w, in);
  if (n > 0) {
    hipLaunchKernelGGL(k_cluster_insert, blocks(n), dim3(kClusterBlock), 0, st, w, in);
    hipLaunchKernelGGL(k_cluster_seed, blocks(n), dim3(kClusterBlock), 0, st, w, in);
    if (connectivity == 6)
      hipLaunchKernelGGL(k_cluster_link<6>, blocks(n), dim3(kClusterBlock), 0, st, w, in);
    else if (connectivity == 18)
      hipLaunchKernelGGL(k_cluster_link<18>, blocks(n), dim3(kClusterBlock), 0, st, w, in);
    else
      hipLaunchKernelGGL(k_cluster_link<26>, blocks(n), dim3(kClusterBlock), 0, st, w, in);
    hipLaunchKernelGGL(k_cluster_flatten, blocks(n), dim3(kClusterBlock), 0, st, w, in);
  }
  hipLaunchKernelGGL(k_cluster_number, dim3(1), dim3(kClusterScanBlock), 0, st, w, in, o, min_size);
  if (n > 0) {
    hipLaunchKernelGGL(k_cluster_reduce, blocks(n), dim3(kClusterBlock), 0, st, w, in, o);
    if (C > 0) hipLaunchKernelGGL(k_cluster_finish, blocks(C), dim3(kClusterBlock), 0, st, w, o, res, org[0], org[1], org[2]);
  }
  FIESTA_HIP_CHECK(hipGetLastError());
}

// Both variants of the call on a map's stream; res / org: the map's resolution and origin -- nothing else of a map is read, so
// both stores share this function.  The device variant only enqueues.  The host variant stages the inputs through P.in and every
// output through P.out, synchronises, reads the totals and copies back the labels and min(total, capacity) of each cluster array.
inline void cluster_voxels_run(hipStream_t st, PlannerScratch &P, double res, const double *org, const ClusterArgs &a) {
  ClusterScratch &S = P.cluster;
  const fiesta_hip_cluster_result none{};
  const fiesta_hip_cluster_result &r = a.res ? *a.res : none;
  if (a.dev) {
    const ClusterIn ci{a.vox, a.mask, a.key, a.n_dev, a.n};
    const ClusterOut co{r.label, r.size, r.root, r.box_lo, r.box_hi, r.centroid, r.mask_or, r.key_min, r.key_argmin, r.offsets, r.members, a.info,
                        a.cluster_capacity, a.member_capacity};
    cluster_enqueue(st, S, ci, co, a.connectivity, a.min_size, res, org);
    return;
  }
  const size_t n = (size_t)a.n, C = (size_t)std::min<int64_t>(a.n, a.cluster_capacity), M = (size_t)std::min<int64_t>(a.n, a.member_capacity);
  Staging in{P.in, st}, out{P.out, st};
  const auto vox = in.add(a.vox, 3 * n), key = in.add(a.key, n);
  const auto mask = in.add(a.mask, n);
  in.alloc(), in.up(vox, 3 * n), in.up(key, n), in.up(mask, n);
  const ClusterIn ci{in.dev(vox), in.dev(mask), in.dev(key), nullptr, a.n};
  const auto info = out.add(a.info, 1);
  const auto root = out.add(r.root, C), key_argmin = out.add(r.key_argmin, C), offsets = out.add(r.offsets, C + 1), members = out.add(r.members, M);
  const auto centroid = out.add(r.centroid, 3 * C);
  const auto label = out.add(r.label, n), size = out.add(r.size, C), box_lo = out.add(r.box_lo, 3 * C), box_hi = out.add(r.box_hi, 3 * C),
             key_min = out.add(r.key_min, C);
  const auto mask_or = out.add(r.mask_or, C);
  out.alloc();
  const ClusterOut co{out.dev(label),   out.dev(size),    out.dev(root),       out.dev(box_lo),  out.dev(box_hi),  out.dev(centroid), out.dev(mask_or),
                      out.dev(key_min), out.dev(key_argmin), out.dev(offsets), out.dev(members), out.dev(info),    (int64_t)C,        (int64_t)M};
  cluster_enqueue(st, S, ci, co, a.connectivity, a.min_size, res, org);
  out.back(info, 1), out.back(label, n);
  FIESTA_HIP_CHECK(hipStreamSynchronize(st));
  const size_t k = (size_t)std::min<int64_t>(a.info->n_clusters, (int64_t)C), mm = (size_t)std::min<int64_t>(a.info->n_members, (int64_t)M);
  out.back(size, k), out.back(root, k), out.back(box_lo, 3 * k), out.back(box_hi, 3 * k), out.back(centroid, 3 * k), out.back(mask_or, k);
  out.back(key_min, k), out.back(key_argmin, k), out.back(offsets, k + 1), out.back(members, mm);
  FIESTA_HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace
}  // namespace fiesta
