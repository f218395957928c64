// fiesta_amd/csrc/reach_matrix_kernels.hpp -- reach matrix: fiesta_hip_reach_matrix / _dev (include/fiesta_hip.h).
//
// A planner that has to ORDER its sites needs the travel cost between every pair of them: row s of the matrix is the flood of
// fiesta_hip_reach_field from source s alone, read at the columns.  One reach_field call per site would rebuild the same
// traversability bitmap K times and run K chains of small launches; here the K floods run side by side over one bitmap:
//   k_reach_mask<SRC>   (reach_kernels.hpp, unchanged) ONCE per call: the box's bitmap and the traversable count; the cost field it
//                       initialises on the way is plane 0 of the first batch
//   k_rmx_init          the bitmap expanded into the B cost planes of a batch (-1 / INT32_MAX), k_reach_mask's half-wave stores
//   k_rmx_seed          one lane per source of the batch: status from the bitmap, cost 0 in its OWN plane, wakes its (flood, tile) item
//   k_rmx_relax<CONN>   the hot path: one work-group per active ITEM, a (flood f, tile t) pair packed as f * ntiles + t (B * ntiles <=
//                       B * voxels <= 2^28 fits a u32); the visit itself is reach_relax_tile, k_reach_relax's routine, on plane f
//   k_rmx_gather        one lane per (source of the batch, column): the plane at the column's voxel; -1 rows for unusable sources
//   k_rmx_count         per plane: traversable voxels with a finite cost (only when source_reached is asked for)
// (The kernels are not named k_reach_*: tests/test_reach_rule.py counts the kernels of reach_kernels.hpp by those name prefixes.)
// Flags and lists cover B * ntiles items, double-buffered by round parity; the three rotating length counters work as in
// k_reach_relax.  Rounds are separate launches, kReachChain of them between two reads of the counters: a round costs one launch
// for ALL floods of the batch, and a batch needs as many rounds as its slowest flood, not the sum.  No cooperative launch, no
// waiting of one work-group for another, atomics only on flags, lists and counters, never on costs.
// The planes are independent shortest-path problems over the same bitmap: no work-group reads or writes a plane other than its
// item's, so the argument for the unsynchronised halo (reach_kernels.hpp, above k_reach_relax) holds plane by plane, and so does
// uniqueness: every output has the same bits for any launch shape, batch width and scheduling.
#pragma once
#include <algorithm>
#include <climits>

#include "../../include/fiesta_hip.h"
#include "common.hpp"
#include "planner.hpp"
#include "planner_args.hpp"
#include "reach_kernels.hpp"

namespace fiesta {
namespace {  // (planner.hip alone includes this header; the namespace is part of the kernels' symbol names)

constexpr int64_t kReachMatrixMaxEntries = 1ll << 28;  // of B cost planes (1 GiB of scratch), and of the matrix itself

// planes f0 .. f1 - 1 of `planes` (nvox entries each) from the bitmap: -1 / INT32_MAX.  One lane per word; blockIdx.y strides the planes
__global__ __launch_bounds__(256) void k_rmx_init(ReachBox b, const uint32_t *bits, int32_t *planes, int64_t nvox, int f0, int f1) {
  const int lane = threadIdx.x & 63;
  const int n = b.ex * b.ey * b.nzw;
  // (the trip count is the same for every lane of the work-group: the shuffles below need whole waves)
  for (int base = blockIdx.x * 256; base < n; base += gridDim.x * 256) {
    const int i = base + threadIdx.x;
    uint32_t t = 0;
    int cb = 0, nv = 0;
    if (i < n) {
      const int w = i % b.nzw, row = i / b.nzw;
      nv = min(32, b.ez - 32 * w);
      t = bits[i];
      cb = row * b.ez + 32 * w;
    }
    // the costs of this wave's 64 words, two words per store instruction: 32 consecutive i32 per half wave
    for (int j = 0; j < 32; ++j) {
      const int from = 2 * j + (lane >> 5), k = lane & 31;
      const uint32_t tw = (uint32_t)__shfl((int)t, from);
      const int c = __shfl(cb, from), v = __shfl(nv, from);
      if (k < v) {
        const int32_t val = ((tw >> k) & 1u) ? INT32_MAX : -1;
        for (int f = f0 + (int)blockIdx.y; f < f1; f += (int)gridDim.y) planes[f * nvox + c + k] = val;
      }
    }
  }
}

// (ox, oy, oz): map voxel of box voxel (0, 0, 0); sources / status: of this batch (n <= B entries); plane i is source i's
__global__ __launch_bounds__(256) void k_rmx_seed(ReachBox b, int ox, int oy, int oz, const int32_t *sources, int n, const uint32_t *bits,
                                                  int32_t *planes, int64_t nvox, uint32_t ntiles, int32_t *status, uint32_t *flag, uint32_t *list,
                                                  unsigned long long *ctr) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  bool usable = false;
  if (i < n) {
    const int64_t x = (int64_t)sources[3 * i] - ox, y = (int64_t)sources[3 * i + 1] - oy, z = (int64_t)sources[3 * i + 2] - oz;
    const bool in = x >= 0 && x < b.ex && y >= 0 && y < b.ey && z >= 0 && z < b.ez;
    if (in) usable = (bits[((int)x * b.ey + (int)y) * b.nzw + ((int)z >> 5)] >> ((int)z & 31)) & 1u;
    status[i] = usable ? FIESTA_HIP_REACH_SITE_OK : (in ? FIESTA_HIP_REACH_SITE_BLOCKED : FIESTA_HIP_REACH_SITE_OUTSIDE);
    if (usable) {
      planes[i * nvox + (x * b.ey + y) * b.ez + z] = 0;
      activate_tile((uint32_t)i * ntiles + (uint32_t)((((int)x >> 4) * b.nty + ((int)y >> 4)) * b.nzw + ((int)z >> 5)), flag, list, &ctr[R_LIST0]);
    }
  }
  const unsigned long long m = __ballot(usable);
  if (m && (int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(&ctr[R_SEEDS], (unsigned long long)__popcll(m));
}

// One round of every flood of the batch.  reach_relax_tile's comment holds plane by plane: an item stages, relaxes and writes plane
// f only, and wakes items of flood f only.
template <int CONN>
__global__ __launch_bounds__(256) void k_rmx_relax(ReachBox b, const uint32_t *bits, int32_t *planes, int64_t nvox, uint32_t ntiles, ReachRound r) {
  const unsigned count = (unsigned)r.ctr[r.cur];  // (nothing appends to this round's own list)
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    r.ctr[r.clear] = 0;
    if (count) atomicAdd(&r.ctr[R_ROUNDS], 1ull);
  }
  for (unsigned it = blockIdx.x; it < count; it += gridDim.x) {
    const uint32_t item = r.list_cur[it], f = item / ntiles;
    reach_relax_tile<CONN>(b, bits, planes + f * nvox, r, (int)(item - f * ntiles), f * ntiles);
  }
}

// cols: n_cols x 3 map voxels; status / out: of this batch's first source (out: n x n_cols, row-major)
__global__ __launch_bounds__(256) void k_rmx_gather(ReachBox b, int ox, int oy, int oz, const int32_t *cols, int64_t n_cols, int n,
                                                    const int32_t *status, const int32_t *planes, int64_t nvox, int32_t *out) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n * n_cols) return;
  const int64_t s = i / n_cols, j = i - s * n_cols;
  int32_t c = -1;
  if (status[s] == FIESTA_HIP_REACH_SITE_OK) {
    const int64_t x = (int64_t)cols[3 * j] - ox, y = (int64_t)cols[3 * j + 1] - oy, z = (int64_t)cols[3 * j + 2] - oz;
    if (x >= 0 && x < b.ex && y >= 0 && y < b.ey && z >= 0 && z < b.ez) c = planes[s * nvox + (x * b.ey + y) * b.ez + z];
  }
  out[i] = c;
}

// reached[f] += voxels of plane f = blockIdx.y with a finite cost (k_reach_stats' reduction)
__global__ __launch_bounds__(256) void k_rmx_count(const int32_t *planes, int64_t nvox, unsigned long long *reached) {
  const int32_t *cost = planes + blockIdx.y * nvox;
  int cnt = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nvox; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = cost[i];
    if (c >= 0 && c != INT32_MAX) ++cnt;
  }
  cnt = wave_sum(cnt);
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&reached[blockIdx.y], (unsigned long long)cnt);
}

// Both variants of the call on a map's stream; lo / hi / off as for reach_run.  Both variants synchronise.
// Neither ReachScratch::cost nor field_valid is touched: what fiesta_hip_reach_paths retains stays as it was.
// What fiesta_hip_leg_paths descends (ReachMatrixScratch::batch_*) is cleared on entry and set by a call that ends in one batch.
template <class SRC>
void reach_matrix_run(hipStream_t st, PlannerScratch &P, const SRC &src, const int64_t lo[3], const int64_t hi[3], const int off[3],
                      const ReachMatrixArgs &a) {
  ReachMatrixScratch &S = P.reach_matrix;
  const fiesta_hip_reach_matrix_result &res = *a.res;
  const int64_t n = a.n_sources, n_cols = a.targets ? a.n_targets : n;
  S.batch_valid = false, S.batch_why = ReachMatrixScratch::kNothingToKeep;  // (fiesta_hip_leg_paths' retained batch: set at the very end)
  if (a.info) *a.info = fiesta_hip_reach_matrix_info{};
  const bool want_cost = res.cost && n > 0 && n_cols > 0;
  // the staged inputs and the staged matrix of the host variant
  const int32_t *dsources = a.sources, *dcols = a.targets ? a.targets : a.sources;
  int32_t *dout = res.cost;
  if (!a.dev) {
    const size_t sb = (size_t)n * 3 * sizeof(int32_t), tb = a.targets ? (size_t)a.n_targets * 3 * sizeof(int32_t) : 0;
    P.in.ensure(sb + tb + 8, st);
    if (want_cost) P.out.ensure((size_t)(n * n_cols) * sizeof(int32_t), st), dout = (int32_t *)P.out.p;
    if (sb) FIESTA_HIP_CHECK(hipMemcpyAsync(P.in.p, a.sources, sb, hipMemcpyHostToDevice, st));
    if (tb) FIESTA_HIP_CHECK(hipMemcpyAsync(P.in.p + sb, a.targets, tb, hipMemcpyHostToDevice, st));
    dsources = (const int32_t *)P.in.p, dcols = tb ? (const int32_t *)(P.in.p + sb) : dsources;
  }
  if (n > 0) {
    S.status.ensure((size_t)n, st);
    S.reached.ensure((size_t)n, st);
    FIESTA_HIP_CHECK(hipMemsetAsync(S.reached.p, 0, (size_t)n * sizeof(unsigned long long), st));
  }
  const hipMemcpyKind back = a.dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  auto results_back = [&] {  // (also the call's synchronisation)
    if (want_cost && !a.dev) FIESTA_HIP_CHECK(hipMemcpyAsync(res.cost, dout, (size_t)(n * n_cols) * sizeof(int32_t), back, st));
    if (res.source_status && n > 0) FIESTA_HIP_CHECK(hipMemcpyAsync(res.source_status, S.status.p, (size_t)n * sizeof(int32_t), back, st));
    if (res.source_reached && n > 0) FIESTA_HIP_CHECK(hipMemcpyAsync(res.source_reached, S.reached.p, (size_t)n * sizeof(int64_t), back, st));
    FIESTA_HIP_CHECK(hipStreamSynchronize(st));
  };
  if (lo[0] > hi[0] || lo[1] > hi[1] || lo[2] > hi[2]) {  // nothing to flood: no voxel, every source outside
    if (want_cost) {
      hipLaunchKernelGGL(k_reach_fill, dim3((unsigned)((n * n_cols + 255) / 256)), dim3(256), 0, st, dout, n * n_cols, -1);
      FIESTA_HIP_CHECK(hipGetLastError());
    }
    if (n > 0) {
      hipLaunchKernelGGL(k_reach_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, S.status.p, n, FIESTA_HIP_REACH_SITE_OUTSIDE);
      FIESTA_HIP_CHECK(hipGetLastError());
    }
    results_back();
    return;
  }
  const int64_t ex = hi[0] - lo[0] + 1, ey = hi[1] - lo[1] + 1, ez = hi[2] - lo[2] + 1;
  // (each extent is below 2^32, so the first product cannot overflow before it is tested)
  if (ex > kReachMaxVoxels || ey > kReachMaxVoxels || ex * ey > kReachMaxVoxels || ex * ey * ez > kReachMaxVoxels)
    throw Error(FIESTA_HIP_ERR_INVALID, "reach_matrix: the clipped box holds more than 2^28 voxels");
  const int64_t nvox = ex * ey * ez;
  ReachBox b{(int)lo[0], (int)lo[1], (int)lo[2], (int)ex, (int)ey, (int)ez, (int)((ez + 31) / 32), (int)((ex + 15) / 16), (int)((ey + 15) / 16)};
  const int64_t nwords = ex * ey * b.nzw, ntiles = (int64_t)b.ntx * b.nty * b.nzw;
  const int ox = (int)(lo[0] + off[0]), oy = (int)(lo[1] + off[1]), oz = (int)(lo[2] + off[2]);
  // the batch width: the caller's bound, the number of sources, and B * nvox <= 2^28 cost entries; at least one plane
  int64_t B = std::max<int64_t>(1, kReachMatrixMaxEntries / nvox);
  if (a.max_fields > 0) B = std::min<int64_t>(B, a.max_fields);
  B = std::max<int64_t>(1, std::min(B, n));
  // scratch, owned by the map (an allocation failure is FIESTA_HIP_ERR_NOMEM and leaves what there was)
  P.reach.bits.ensure_exact((size_t)nwords, st);  // (the reach_field bitmap: nothing retains it)
  S.planes.ensure_exact((size_t)(B * nvox), st);
  S.flags.ensure((size_t)(2 * B * ntiles), st);
  S.lists.ensure((size_t)(2 * B * ntiles), st);
  S.ctr.ensure(R_COUNT, st);
  const uint32_t *bits = P.reach.bits.p;
  FIESTA_HIP_CHECK(hipMemsetAsync(S.ctr.p, 0, R_COUNT * sizeof(unsigned long long), st));
  FIESTA_HIP_CHECK(hipMemsetAsync(S.flags.p, 0, (size_t)(2 * B * ntiles) * sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_reach_mask<SRC>, dim3(reach_blocks(nwords, 256, 8192)), dim3(256), 0, st, src, b, a.min_clearance,
                     (a.flags & FIESTA_HIP_REACH_THROUGH_UNKNOWN) ? 1 : 0, P.reach.bits.p, S.planes.p, S.ctr.p);
  FIESTA_HIP_CHECK(hipGetLastError());
  uint32_t *flag[2] = {S.flags.p, S.flags.p + B * ntiles}, *list[2] = {S.lists.p, S.lists.p + B * ntiles};
  unsigned long long h[R_COUNT];
  auto read_counters = [&] {
    FIESTA_HIP_CHECK(hipMemcpyAsync(h, S.ctr.p, sizeof(h), hipMemcpyDeviceToHost, st));
    FIESTA_HIP_CHECK(hipStreamSynchronize(st));
  };
  int64_t batches = 0;
  for (int64_t s0 = 0; s0 < n; s0 += B, ++batches) {
    const int nb = (int)std::min<int64_t>(B, n - s0);
    const int f0 = s0 == 0 ? 1 : 0;  // (k_reach_mask has written plane 0 of the first batch)
    if (s0 > 0) FIESTA_HIP_CHECK(hipMemsetAsync(S.ctr.p, 0, 3 * sizeof(unsigned long long), st));  // R_LIST0 .. R_LIST2: the rounds restart at 0
    if (f0 < nb) {
      hipLaunchKernelGGL(k_rmx_init, dim3(reach_blocks(nwords, 256, 2048), (unsigned)std::min(nb - f0, 64)), dim3(256), 0, st, b, bits, S.planes.p,
                         nvox, f0, nb);
      FIESTA_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_rmx_seed, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, b, ox, oy, oz, dsources + 3 * s0, nb, bits, S.planes.p, nvox,
                       (uint32_t)ntiles, S.status.p + s0, flag[0], list[0], S.ctr.p);
    FIESTA_HIP_CHECK(hipGetLastError());
    const int groups = (int)std::min<int64_t>(nb * ntiles, kReachMaxGroups);
    const unsigned long long rounds_before = batches ? h[R_ROUNDS] : 0ull;
    for (int64_t round = 0;;) {
      for (int k = 0; k < kReachChain; ++k, ++round) {
        const int p = (int)(round & 1);
        const ReachRound rr{flag[p], flag[p ^ 1], list[p], list[p ^ 1], S.ctr.p, R_LIST0 + (int)(round % 3), R_LIST0 + (int)((round + 1) % 3),
                            R_LIST0 + (int)((round + 2) % 3)};
        if (a.connectivity == 6)
          hipLaunchKernelGGL(k_rmx_relax<6>, dim3(groups), dim3(256), 0, st, b, bits, S.planes.p, nvox, (uint32_t)ntiles, rr);
        else
          hipLaunchKernelGGL(k_rmx_relax<26>, dim3(groups), dim3(256), 0, st, b, bits, S.planes.p, nvox, (uint32_t)ntiles, rr);
        FIESTA_HIP_CHECK(hipGetLastError());
      }
      read_counters();
      if (h[R_LIST0 + round % 3] == 0) break;
      // after round r every voxel whose shortest path crosses fewer than r tile faces is final: more rounds than voxels is a bug
      if (h[R_ROUNDS] - rounds_before > h[R_NTRAV] + 1) throw Error(FIESTA_HIP_ERR_STATE, "reach_matrix: a batch of floods did not settle");
    }
    if (want_cost) {
      hipLaunchKernelGGL(k_rmx_gather, dim3((unsigned)((nb * n_cols + 255) / 256)), dim3(256), 0, st, b, ox, oy, oz, dcols, n_cols, nb,
                         (const int32_t *)(S.status.p + s0), (const int32_t *)S.planes.p, nvox, dout + s0 * n_cols);
      FIESTA_HIP_CHECK(hipGetLastError());
    }
    if (res.source_reached) {
      hipLaunchKernelGGL(k_rmx_count, dim3(reach_blocks(nvox, 256 * 16, 512), (unsigned)nb), dim3(256), 0, st, (const int32_t *)S.planes.p, nvox,
                         S.reached.p + s0);
      FIESTA_HIP_CHECK(hipGetLastError());
    }
  }
  if (n == 0) read_counters();  // (the traversable count alone)
  // one batch: plane s is source s's flood and stays so until the next call -- the batch fiesta_hip_leg_paths descends.  The sources
  // are copied: the caller's array may be freed, the host variant's staging is the next call's
  const bool keep = n > 0 && batches == 1;
  if (keep) {
    S.sites.ensure((size_t)(3 * n), st);
    FIESTA_HIP_CHECK(hipMemcpyAsync(S.sites.p, dsources, (size_t)(3 * n) * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  }
  results_back();
  if (keep) {
    S.batch_lo[0] = ox, S.batch_lo[1] = oy, S.batch_lo[2] = oz;
    for (int c = 0; c < 3; ++c) S.batch_hi[c] = (int32_t)(hi[c] + off[c]);
    S.batch_connectivity = a.connectivity, S.batch_sources = n;
    S.batch_valid = true;
  } else if (n > 0) {
    S.batch_why = ReachMatrixScratch::kManyBatches;
  }
  if (a.info) {
    fiesta_hip_reach_matrix_info &I = *a.info;
    I.box_lo[0] = ox, I.box_lo[1] = oy, I.box_lo[2] = oz;
    I.box_hi[0] = (int32_t)(hi[0] + off[0]), I.box_hi[1] = (int32_t)(hi[1] + off[1]), I.box_hi[2] = (int32_t)(hi[2] + off[2]);
    I.n_traversable = (int64_t)h[R_NTRAV], I.n_sources_used = (int64_t)h[R_SEEDS];
    I.fields = n > 0 ? B : 0, I.batches = batches;
    I.rounds = (int64_t)h[R_ROUNDS], I.tile_visits = (int64_t)h[R_VISITS];
  }
}

}  // namespace
}  // namespace fiesta
