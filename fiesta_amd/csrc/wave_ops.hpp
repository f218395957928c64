// fiesta_amd/csrc/wave_ops.hpp -- the wave and work-group primitives of the planner kernels (device only).
//
//   wave_reduce / wave_sum / wave_min / wave_max / wave_or   the xor butterfly over the 64 lanes, the result in every lane
//   wave_inclusive / wave_inclusive_sum                      the __shfl_up scan over the 64 lanes
//   block_inclusive                                          the same over a work-group: wave totals through LDS
//   block_scan_stride                                        ONE work-group scans a whole array, the carry in a register
//   wave_for_each_key / wave_count_keys                      serve the DISTINCT keys present in a wave, one trip per key
//   VoxelBox / VoxelStats / VoxelAcc                         per-key voxel statistics: wave aggregate, accumulators, output
// Every function here must be called by WHOLE waves (all 64 lanes reach the call together); the block_ ones by every lane of the
// work-group, in uniform control flow (they hold barriers).  The UpdateESDF engines do not use this header.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <climits>

namespace fiesta {
namespace {  // (included by several translation units)

struct WaveSum {
  template <class T>
  __device__ T operator()(T a, T b) const { return a + b; }
};
struct WaveMin {
  template <class T>
  __device__ T operator()(T a, T b) const { return a < b ? a : b; }
};
struct WaveMax {
  template <class T>
  __device__ T operator()(T a, T b) const { return a > b ? a : b; }
};
struct WaveOr {
  template <class T>
  __device__ T operator()(T a, T b) const { return a | b; }
};

// v reduced over the wave; every lane returns the same bits (op is commutative: both partners of a butterfly step compute the same
// value)
template <class T, class Op>
__device__ inline T wave_reduce(T v, Op op) {
  for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
  return v;
}
template <class T>
__device__ inline T wave_sum(T v) { return wave_reduce(v, WaveSum{}); }
template <class T>
__device__ inline T wave_min(T v) { return wave_reduce(v, WaveMin{}); }
template <class T>
__device__ inline T wave_max(T v) { return wave_reduce(v, WaveMax{}); }
template <class T>
__device__ inline T wave_or(T v) { return wave_reduce(v, WaveOr{}); }

// inclusive scan over the lanes of the wave; the wave's total is __shfl(result, 63)
template <class T, class Op>
__device__ inline T wave_inclusive(T v, Op op) {
  const int lane = threadIdx.x & 63;
  for (int o = 1; o < 64; o <<= 1) {
    const T u = __shfl_up(v, o, 64);
    if (lane >= o) v = op(v, u);
  }
  return v;
}
template <class T>
__device__ inline T wave_inclusive_sum(T v) { return wave_inclusive(v, WaveSum{}); }

// Inclusive scan of one value per thread over the work-group; *total = the whole group's.  lds: one word per wave.  The second
// barrier frees lds for the next call.  NWAVES: the work-group's wave count (every caller's is a constant).
template <int NWAVES, class T, class Op>
__device__ inline T block_inclusive(T v, T ident, Op op, T *lds, T *total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  v = wave_inclusive(v, op);
  if (lane == 63) lds[wv] = v;
  __syncthreads();
  T pre = ident, tot = ident;
  for (int k = 0; k < NWAVES; ++k) {
    if (k < wv) pre = op(pre, lds[k]);
    tot = op(tot, lds[k]);
  }
  __syncthreads();
  *total = tot;
  return op(pre, v);
}

// ONE work-group sums over items [0, n), ITEMS consecutive items per lane and trip, the carry in a register.  load(i) gives item
// i's value; store(i, excl, v) receives the sum of the items before i and the value load gave.  Both are called for i < n only,
// load for every item of a trip before any store of it.  Returns the total, in every lane.  (The same trip count for every lane:
// the barriers need all of them.)
template <int ITEMS, int NWAVES, class T, class Load, class Store>
__device__ inline T block_scan_stride(int64_t n, T *lds, Load load, Store store) {
  T carry = 0;
  for (int64_t base = 0; base < n; base += (int64_t)NWAVES * 64 * ITEMS) {
    const int64_t i0 = base + (int64_t)threadIdx.x * ITEMS;
    T x[ITEMS], sum = 0;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) x[k] = i0 + k < n ? load(i0 + k) : (T)0, sum += x[k];
    T total;
    T run = carry + block_inclusive<NWAVES>(sum, (T)0, WaveSum{}, lds, &total) - sum;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
      if (i0 + k < n) store(i0 + k, run, x[k]);
      run += x[k];
    }
    carry += total;
  }
  return carry;
}

// Serves the distinct keys among the wave's `active` lanes: per key one call body(key, mine, same) in every lane -- mine: this lane
// holds the key; same: the ballot of such lanes.  The trip count is the number of distinct keys, uniform across the wave.
template <class Body>
__device__ inline void wave_for_each_key(bool active, int key, Body body) {
  unsigned long long todo = __ballot(active);
  while (todo) {
    const int k = __shfl(key, __ffsll((long long)todo) - 1);
    const bool mine = active && key == k;
    const unsigned long long same = __ballot(mine);
    todo &= ~same;
    body(k, mine, same);
  }
}
__device__ inline bool wave_first_of(unsigned long long same) { return (int)(threadIdx.x & 63) == __ffsll((long long)same) - 1; }
// acc[key] += the number of active lanes with that key: one atomicAdd per wave and distinct key
__device__ inline void wave_count_keys(int32_t *acc, bool active, int key) {
  wave_for_each_key(active, key, [&](int k, bool, unsigned long long same) {
    if (wave_first_of(same)) atomicAdd(&acc[k], __popcll(same));
  });
}

// ---- per-key voxel statistics ----------------------------------------------------------------------------------------------------
// A lane's share of one key's statistics: the voxel of a lane that holds the key, the identity in every other lane.  reduce() is the
// butterfly (afterwards every lane holds the wave's aggregate), commit() the atomics: ONE per quantity, by the lane the caller picks.
struct VoxelBox {
  int lx, ly, lz, hx, hy, hz;
  __device__ static VoxelBox at(bool mine, int x, int y, int z) {
    return VoxelBox{mine ? x : INT32_MAX, mine ? y : INT32_MAX, mine ? z : INT32_MAX, mine ? x : INT32_MIN, mine ? y : INT32_MIN, mine ? z : INT32_MIN};
  }
  __device__ static VoxelBox identity() { return at(false, 0, 0, 0); }
  __device__ void combine(const VoxelBox &o) {
    lx = min(lx, o.lx), ly = min(ly, o.ly), lz = min(lz, o.lz), hx = max(hx, o.hx), hy = max(hy, o.hy), hz = max(hz, o.hz);
  }
  __device__ VoxelBox partner(int off) const {
    return VoxelBox{__shfl_xor(lx, off), __shfl_xor(ly, off), __shfl_xor(lz, off), __shfl_xor(hx, off), __shfl_xor(hy, off), __shfl_xor(hz, off)};
  }
  __device__ void reduce() {
    for (int off = 32; off >= 1; off >>= 1) combine(partner(off));
  }
  __device__ void commit(int32_t *b) const {  // b: the key's six words, min x, y, z, max x, y, z
    atomicMin(b, lx), atomicMin(b + 1, ly), atomicMin(b + 2, lz), atomicMax(b + 3, hx), atomicMax(b + 4, hy), atomicMax(b + 5, hz);
  }
  __device__ static void reset(int32_t *b) { b[0] = b[1] = b[2] = INT32_MAX, b[3] = b[4] = b[5] = INT32_MIN; }
};

// the accumulators of keys 0 .. : exact coordinate sums (two's complement), box, mask OR, the packed (key << 32 | index) minimum
struct VoxelAcc {
  unsigned long long *sum;   // 3 per key
  int32_t *box;              // 6 per key
  uint32_t *mor;             // 1
  unsigned long long *kmin;  // 1 (~0: none)
  __device__ void reset(int64_t k) const {
    sum[3 * k] = sum[3 * k + 1] = sum[3 * k + 2] = 0;
    VoxelBox::reset(box + 6 * k);
    mor[k] = 0, kmin[k] = ~0ull;
  }
};
struct VoxelStatsOut {  // device pointers, every one nullable
  int32_t *box_lo, *box_hi;
  double *centroid;
  uint8_t *mask_or;
  int32_t *key_min;
  int64_t *key_argmin;
};

struct VoxelStats {  // (a wave's coordinate sum fits 32 bits: 64 * 2^20)
  int sx, sy, sz;
  VoxelBox box;
  uint32_t mask;
  unsigned long long kmin;
  // mk: the voxel's mask; kp: its packed (key << 32 | index), ~0 without a key
  __device__ static VoxelStats at(bool mine, int x, int y, int z, uint32_t mk, unsigned long long kp) {
    return VoxelStats{mine ? x : 0, mine ? y : 0, mine ? z : 0, VoxelBox::at(mine, x, y, z), mine ? mk : 0u, mine ? kp : ~0ull};
  }
  __device__ void combine(const VoxelStats &o) {
    sx += o.sx, sy += o.sy, sz += o.sz;
    box.combine(o.box);
    mask |= o.mask;
    kmin = o.kmin < kmin ? o.kmin : kmin;
  }
  __device__ void reduce() {
    for (int off = 32; off >= 1; off >>= 1)
      combine(VoxelStats{__shfl_xor(sx, off), __shfl_xor(sy, off), __shfl_xor(sz, off), box.partner(off), __shfl_xor(mask, off), __shfl_xor(kmin, off)});
  }
  __device__ void commit(const VoxelAcc &a, int64_t k) const {
    atomicAdd(&a.sum[3 * k], (unsigned long long)(long long)sx);
    atomicAdd(&a.sum[3 * k + 1], (unsigned long long)(long long)sy);
    atomicAdd(&a.sum[3 * k + 2], (unsigned long long)(long long)sz);
    box.commit(a.box + 6 * k);
    if (mask) atomicOr(&a.mor[k], mask);
    if (kmin != ~0ull) atomicMin(&a.kmin[k], kmin);
  }
};

// the outputs of key k out of its accumulators (size > 0: its voxel count); the centroid in the operation order of reach_path_store
// (no contraction: -ffp-contract=off)
__device__ inline void voxel_stats_write(const VoxelAcc &a, const VoxelStatsOut &o, int64_t k, int size, double res, double ox, double oy, double oz) {
  const int32_t *b = a.box + 6 * k;
  if (o.box_lo) o.box_lo[3 * k] = b[0], o.box_lo[3 * k + 1] = b[1], o.box_lo[3 * k + 2] = b[2];
  if (o.box_hi) o.box_hi[3 * k] = b[3], o.box_hi[3 * k + 1] = b[4], o.box_hi[3 * k + 2] = b[5];
  if (o.centroid) {
    const double org[3] = {ox, oy, oz};
#pragma unroll
    for (int c = 0; c < 3; ++c) o.centroid[3 * k + c] = ((double)(long long)a.sum[3 * k + c] / (double)size + 0.5) * res + org[c];
  }
  if (o.mask_or) o.mask_or[k] = (uint8_t)a.mor[k];
  const unsigned long long kk = a.kmin[k];
  if (o.key_min) o.key_min[k] = kk == ~0ull ? INT32_MAX : (int32_t)(kk >> 32);
  if (o.key_argmin) o.key_argmin[k] = kk == ~0ull ? -1 : (int64_t)(kk & 0xFFFFFFFFull);
}

}  // namespace
}  // namespace fiesta
