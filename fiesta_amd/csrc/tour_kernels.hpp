// fiesta_amd/csrc/tour_kernels.hpp -- site tour: fiesta_hip_site_tour / _dev (include/fiesta_hip.h).
//
// The last step of the planner chain frontier voxels -> clusters -> views -> reach matrix: ORDER the sites.  A restart-parallel
// best-improvement local search (2-opt, Or-opt of 1 / 2 / 3 sites) over the sites the start can reach; the contract, word for word,
// is the header's, fiesta_amd.tour_model is the definition, and every output is held to its bits.
//   k_tour_prepare        the visited list (the start first, then ascending), the statuses, the two checks among visited sites
//                         (every pair a connection, the matrix symmetric) into two error words, the compact m x m matrix
//   k_tour_search<IN_LDS> the hot path: one work-group per restart; the tour, the leg costs C(k, k + 1) and a scratch array live in
//                         LDS, and for m <= kTourLdsSites = 128 the matrix too (64 KiB: with the small arrays 66 KiB, two
//                         work-groups per CU); above that it is read from the compact copy (1 MiB at most: L2-resident)
//   k_tour_pick           the arg-min over restarts, local -> site indices, order / leg_cost / site_status / restart_length, the info
// (The kernels are not named k_reach_*: tests/test_reach_rule.py counts the kernels of reach_kernels.hpp by those name prefixes.)
// One iteration of the search: the lanes split the flat move space (type, i, x) -- 4 (m - 1) m keys, lane l takes l, l + 256, ..
// without a division, four keys per trip with every read unconditional so that their LDS latencies overlap -- each keeps the
// least packed word (delta + 2^34) << 22 | type << 20 | i << 10 | x (|delta| < 3 * 2^31, so the order of the words is "most
// negative delta, then lowest key": the contract's tie rule survives any reduction order), the work-group reduces wave first
// (shuffles), then through four LDS words, and all lanes apply the winner together: every lane reads the element that lands on
// its position, barrier, writes it.
// LDS banks: with the legs C(k, k + 1) kept in an array (read at consecutive k: conflict-free) every remaining matrix read of a
// lane group has one fixed row per (type, i) (the matrix is symmetric, so C(p, i) is read as row t[i]) and the columns t[x] of
// consecutive x.
// The columns of a lane group are distinct entries of a permutation, so two lanes share a bank iff their columns agree mod 32
// (ds_read_b32: bank = dword address mod 32 per 32-lane half), whatever the row stride: padding the rows changes nothing, and the
// matrix is stored dense with stride m.
// Work-group size 256: four waves, one per SIMD of a CU; the move space of a planner-sized tour (32 sites: 3968 keys, 64 sites:
// 16128) is 16 to 63 keys per lane, and the four barriers per iteration (legs, reduce, apply's two) stay among four waves.  Nothing waits for
// another work-group, the only stores to global memory are plain ones to the restart's own slots.
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

constexpr int kTourThreads = 256;
constexpr int kTourLdsSites = 128;  // the matrix lives in LDS up to this m
// TourScratch::head, int32 words: m, the two error words, then (8-byte aligned) the info struct and the nearest-neighbour length
enum { TH_M = 0, TH_ERR_CONN = 1, TH_ERR_SYM = 2, TH_INFO = 4, TH_NN = 16, TH_WORDS = 32 };
constexpr unsigned long long kTourNoMove = 1ull << 56;  // the packed word of (delta 0, key 0): every improving move is below it

__device__ inline bool tour_connection(int32_t c) { return c >= 0 && c != INT32_MAX; }

__device__ inline unsigned long long tour_mix(unsigned long long x) {
  x ^= x >> 30, x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27, x *= 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// the work-group's minimum / sum, wave first, then through red[2][4] (alternating halves: one barrier per call, which also
// orders the LDS traffic around it)
__device__ inline unsigned long long tour_block_min(unsigned long long v, unsigned long long *red, int &par) {
  v = wave_min(v);
  if ((threadIdx.x & 63) == 0) red[par * 4 + (threadIdx.x >> 6)] = v;
  __syncthreads();
  unsigned long long r = red[par * 4];
  for (int w = 1; w < kTourThreads / 64; ++w) r = red[par * 4 + w] < r ? red[par * 4 + w] : r;
  par ^= 1;
  return r;
}
__device__ inline long long tour_block_sum(long long v, unsigned long long *red, int &par) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[par * 4 + (threadIdx.x >> 6)] = (unsigned long long)v;
  __syncthreads();
  long long r = 0;
  for (int w = 0; w < kTourThreads / 64; ++w) r += (long long)red[par * 4 + w];
  par ^= 1;
  return r;
}

// grid: any number of work-groups; each builds the visited list for itself and takes every gridDim.x-th row of the compact matrix
__global__ __launch_bounds__(kTourThreads) void k_tour_prepare(const int32_t *cost, int n, long long ld, int start, int32_t *head, int32_t *site,
                                                               int32_t *status, int32_t *mat) {
  __shared__ int vis[FIESTA_HIP_TOUR_MAX_SITES], lsite[FIESTA_HIP_TOUR_MAX_SITES];
  __shared__ int s_m;
  const int tid = threadIdx.x;
  for (int j = tid; j < n; j += kTourThreads) vis[j] = (j == start || tour_connection(cost[start * ld + j])) ? 1 : 0;
  __syncthreads();
  for (int j = tid; j < n; j += kTourThreads) {
    if (!vis[j] || j == start) continue;
    int rank = 1;
    for (int k = 0; k < j; ++k) rank += (vis[k] && k != start) ? 1 : 0;
    lsite[rank] = j;
  }
  if (tid == 0) {
    int m = 0;
    for (int k = 0; k < n; ++k) m += vis[k];
    s_m = m, lsite[0] = start;
  }
  __syncthreads();
  const int m = s_m;
  bool no_conn = false, asym = false;
  for (int la = blockIdx.x; la < m; la += gridDim.x) {
    const long long a = lsite[la];
    for (int lb = tid; lb < m; lb += kTourThreads) {
      const long long b = lsite[lb];
      const int32_t c = cost[a * ld + b];
      if (la != lb) no_conn |= !tour_connection(c), asym |= c != cost[b * ld + a];
      mat[la * m + lb] = la == lb ? 0 : c;
    }
  }
  if (no_conn) head[TH_ERR_CONN] = 1;  // (plain stores of one value: the words were cleared before the launch)
  if (asym) head[TH_ERR_SYM] = 1;
  if (blockIdx.x == 0) {
    if (tid == 0) head[TH_M] = m;
    for (int j = tid; j < n; j += kTourThreads) status[j] = vis[j] ? FIESTA_HIP_TOUR_SITE_VISITED : FIESTA_HIP_TOUR_SITE_SKIPPED;
    for (int k = tid; k < m; k += kTourThreads) site[k] = lsite[k];
  }
}

// Restart r = blockIdx.x over the compact matrix gmat (m x m, m >= 1).  tours: R x m local indices; len: R; stat: R x (moves, capped)
template <bool IN_LDS>
__global__ __launch_bounds__(kTourThreads) void k_tour_search(const int32_t *gmat, int m, int closed, unsigned long long seed, int max_moves,
                                                              int32_t *tours, long long *len, int32_t *stat, int32_t *head) {
  constexpr int MAXM = IN_LDS ? kTourLdsSites : FIESTA_HIP_TOUR_MAX_SITES;
  constexpr int PER = (MAXM + kTourThreads - 1) / kTourThreads;  // tour positions per lane
  __shared__ int32_t smat[IN_LDS ? kTourLdsSites * kTourLdsSites : 1];
  __shared__ int t[MAXM + 1], leg[MAXM], scr[MAXM];  // t[m] = t[0]; leg[k] = C(k, k + 1); scr: the initial tours' scratch
  __shared__ unsigned long long red[8];
  const int tid = threadIdx.x, r = blockIdx.x;
  int par = 0;
  if (IN_LDS) {
    for (int k = tid; k < m * m; k += kTourThreads) smat[k] = gmat[k];
    __syncthreads();
  }
  auto M = [&](int a, int b) -> int { return IN_LDS ? smat[a * m + b] : gmat[a * m + b]; };
  // ---- the initial tour
  if (r == 0) {  // nearest neighbour from index 0: the least cost from the last one, ties to the lowest index
    for (int k = tid; k < m; k += kTourThreads) scr[k] = k != 0;
    if (tid == 0) t[0] = 0;
    __syncthreads();
    int last = 0;
    for (int step = 1; step < m; ++step) {
      unsigned long long best = ~0ull;
      for (int k = tid; k < m; k += kTourThreads)
        if (scr[k]) {
          const unsigned long long w = ((unsigned long long)(unsigned)M(last, k) << 32) | (unsigned)k;
          best = w < best ? w : best;
        }
      best = tour_block_min(best, red, par);
      last = (int)(best & 0xffffffffu);
      if (tid == 0) t[step] = last, scr[last] = 0;
      __syncthreads();
    }
  } else {  // the seeded shuffle: the draws in parallel, the swaps in order
    const unsigned long long base = tour_mix(seed + (unsigned long long)r * 0x9E3779B97F4A7C15ull);
    for (int k = tid; k < m; k += kTourThreads) {
      t[k] = k;
      if (k >= 2) scr[k] = 1 + (int)(tour_mix(base + (unsigned long long)k) % (unsigned long long)k);
    }
    __syncthreads();
    if (tid == 0)
      for (int k = m - 1; k >= 2; --k) {
        const int j = scr[k], v = t[k];
        t[k] = t[j], t[j] = v;
      }
  }
  if (tid == 0) t[m] = t[0];
  __syncthreads();
  // C(site at some position, position b): position m is position 0 when closed and dropped when open
  auto Cn = [&](int site, int b) -> long long { return (b == m && !closed) ? 0ll : (long long)M(site, t[b]); };
  auto legs = [&] {  // (ends with a barrier)
    for (int k = tid; k < m; k += kTourThreads) leg[k] = (int)Cn(t[k], k + 1);
    __syncthreads();
  };
  auto length = [&]() -> long long {
    long long s = 0;
    for (int k = tid; k < m; k += kTourThreads) s += leg[k];
    return tour_block_sum(s, red, par);
  };
  legs();
  if (r == 0) {
    const long long nn = length();
    if (tid == 0) *(long long *)(head + TH_NN) = nn;
  }
  // ---- the search
  int moves = 0, capped = 0;
  if (m >= 3) {
    const int rows = 4 * (m - 1), q = kTourThreads / m, rem = kTourThreads % m;
    for (;;) {
      unsigned long long best = kTourNoMove;
      // four keys per trip, every read unconditional (a key past the end or outside its type's range evaluates key (0, 1, .) and is
      // dropped): the LDS reads of the four are independent and overlap, which one work-group per CU needs
      for (int row = tid / m, x = tid % m; row < rows;) {
        constexpr int U = 4;
        int ty[U], i[U], ec[U], xs[U], a1[U], a2[U], a3[U], b1[U], b3[U];
        long long lg[U];  // (three legs: above an int32)
        bool valid[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {  // the keys, then every tour and leg read of the four
          const bool in = row < rows;
          ty[u] = 0, i[u] = in ? row : 0;  // row = type * (m - 1) + (i - 1)
          for (int k = 0; k < 3; ++k)
            if (i[u] >= m - 1) i[u] -= m - 1, ++ty[u];
          ++i[u];
          const int e = ty[u] ? i[u] + ty[u] - 1 : i[u];
          ec[u] = e < m ? e : m - 1, xs[u] = x;
          valid[u] = in && (ty[u] ? (e <= m - 1 && (x < i[u] - 1 || x > e)) : x > i[u]);
          x += rem, row += q;
          if (x >= m) x -= m, ++row;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int ti1 = t[i[u] - 1], ti = t[i[u]], te = t[ec[u]], te1 = t[ec[u] + 1], tx = t[xs[u]], tx1 = t[xs[u] + 1];
          const int li = leg[i[u] - 1], le = leg[ec[u]], lx = leg[xs[u]];
          // 2-opt: C(i-1, j) - C(i-1, i) + C(i, j+1) - C(j, j+1);  Or-opt: C(i-1, e+1) - C(i-1, i) - C(e, e+1) + C(p, i) + C(e, p+1) - C(p, p+1)
          a1[u] = ti1, b1[u] = ty[u] ? te1 : tx, a2[u] = ti, a3[u] = ty[u] ? te : ti, b3[u] = tx1;
          lg[u] = (long long)li + (ty[u] ? le : 0) + lx, xs[u] |= tx << 16;  // (the column of the middle term rides along: tx < 512)
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int c1 = M(a1[u], b1[u]), c2 = M(a2[u], xs[u] >> 16), c3 = M(a3[u], b3[u]);
          const int xx = xs[u] & 0xffff;
          const bool drop_e = !closed && ec[u] + 1 == m, drop_x = !closed && xx + 1 == m;  // the terms that name position m of an open tour
          const long long d = (long long)((ty[u] && drop_e) ? 0 : c1) + (ty[u] ? c2 : 0) + (drop_x ? 0 : c3) - lg[u];
          unsigned long long w = ((unsigned long long)(d + (1ll << 34)) << 22) | ((unsigned long long)ty[u] << 20) | ((unsigned long long)i[u] << 10) | (unsigned)xx;
          w = (valid[u] && d < 0) ? w : kTourNoMove;  // (a select, not a branch: the twelve matrix reads stay in one block)
          best = w < best ? w : best;
        }
      }
      best = tour_block_min(best, red, par);
      if (best == kTourNoMove) break;
      if (moves == max_moves) {
        capped = 1;
        break;
      }
      const int ty = (int)(best >> 20) & 3, i = (int)(best >> 10) & 1023, x = (int)best & 1023;
      const int L = ty, e = i + L - 1;
      int v[PER];
#pragma unroll
      for (int u = 0; u < PER; ++u) {
        const int k = tid + u * kTourThreads;
        int s = k;
        if (ty == 0) {
          if (k >= i && k <= x) s = i + x - k;
        } else if (x < i) {  // the segment moves towards the front: to positions x + 1 .. x + L
          if (k > x && k <= e) s = k <= x + L ? i + (k - (x + 1)) : k - L;
        } else {  // towards the back: to positions x - L + 1 .. x
          if (k >= i && k <= x) s = k <= x - L ? k + L : i + (k - (x - L + 1));
        }
        v[u] = k < m ? t[s] : 0;
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < PER; ++u) {
        const int k = tid + u * kTourThreads;
        if (k < m) t[k] = v[u];
      }
      __syncthreads();
      ++moves;
      legs();
    }
  }
  const long long total = length();
  for (int k = tid; k < m; k += kTourThreads) tours[(long long)r * m + k] = t[k];
  if (tid == 0) len[r] = total, stat[2 * r] = moves, stat[2 * r + 1] = capped;
}

// one work-group: the best restart (least length, then lowest r), its tour in site indices, the legs, the info
__global__ __launch_bounds__(kTourThreads) void k_tour_pick(const int32_t *mat, int m, int n, int closed, int R, const int32_t *tours, const long long *len,
                                                            const int32_t *stat, const int32_t *site, const int32_t *status, int32_t *head,
                                                            fiesta_hip_tour_result out) {
  __shared__ unsigned long long red[8];
  const int tid = threadIdx.x;
  int par = 0;
  unsigned long long best = ~0ull;
  long long moves = 0, capped = 0;
  for (int r = tid; r < R; r += kTourThreads) {
    const unsigned long long w = ((unsigned long long)len[r] << 12) | (unsigned)r;  // (len < 512 * 2^31, r < 4096)
    best = w < best ? w : best;
    moves += stat[2 * r], capped += stat[2 * r + 1];
    if (out.restart_length) out.restart_length[r] = len[r];
  }
  best = tour_block_min(best, red, par);
  moves = tour_block_sum(moves, red, par);
  capped = tour_block_sum(capped, red, par);
  const int b = (int)(best & 4095u);
  const int32_t *t = tours + (long long)b * m;
  for (int k = tid; k < n; k += kTourThreads) {
    if (out.order) out.order[k] = k < m ? site[t[k]] : -1;
    if (out.leg_cost) out.leg_cost[k] = k >= m ? -1 : k > 0 ? mat[t[k - 1] * m + t[k]] : closed ? mat[t[m - 1] * m + t[0]] : 0;
    if (out.site_status) out.site_status[k] = status[k];
  }
  if (tid == 0) {
    fiesta_hip_tour_info *I = (fiesta_hip_tour_info *)(head + TH_INFO);
    I->n_visited = m, I->best_restart = b;
    I->length = (long long)(best >> 12), I->nn_length = *(const long long *)(head + TH_NN);
    I->moves = moves, I->capped = capped;
  }
}

// Both variants of the call on a map's stream; both synchronise (the errors among visited sites are found on the device, and m
// decides the search's instantiation).  No scratch of another call is touched but the staging buffers of a host variant.
inline void site_tour_run(hipStream_t st, PlannerScratch &P, const TourArgs &a) {
  TourScratch &S = P.tour;
  static const fiesta_hip_tour_result none{};
  const fiesta_hip_tour_result &res = a.res ? *a.res : none;
  const int n = a.n, R = a.restarts, closed = (a.flags & FIESTA_HIP_TOUR_CLOSED) ? 1 : 0;
  const int32_t *dcost = a.cost;
  long long ld = a.ld;
  Staging in{P.in, st}, out{P.out, st};
  const auto order = out.add(res.order, n), site_status = out.add(res.site_status, n), leg_cost = out.add(res.leg_cost, n);
  const auto restart_length = out.add(res.restart_length, R);
  fiesta_hip_tour_result dres = res;
  if (!a.dev) {  // the matrix goes up row by row into a dense n x n copy
    const auto c = in.add(a.cost, (size_t)n * n);
    in.alloc(), out.alloc();
    FIESTA_HIP_CHECK(hipMemcpy2DAsync(P.in.p + c.off, (size_t)n * sizeof(int32_t), a.cost, (size_t)a.ld * sizeof(int32_t), (size_t)n * sizeof(int32_t), (size_t)n,
                                      hipMemcpyHostToDevice, st));
    dcost = in.dev(c), ld = n;
    dres = fiesta_hip_tour_result{out.dev(order), out.dev(site_status), out.dev(leg_cost), out.dev(restart_length)};
  }
  S.head.ensure(TH_WORDS, st), S.site.ensure((size_t)n, st), S.status.ensure((size_t)n, st), S.mat.ensure((size_t)n * n, st);
  S.tours.ensure((size_t)R * n, st), S.stat.ensure((size_t)2 * R, st), S.len.ensure((size_t)R, st);
  FIESTA_HIP_CHECK(hipMemsetAsync(S.head.p, 0, TH_WORDS * sizeof(int32_t), st));
  hipLaunchKernelGGL(k_tour_prepare, dim3((unsigned)((n + 15) / 16)), dim3(kTourThreads), 0, st, dcost, n, ld, a.start, S.head.p, S.site.p, S.status.p,
                     S.mat.p);
  FIESTA_HIP_CHECK(hipGetLastError());
  int32_t h[TH_INFO];
  FIESTA_HIP_CHECK(hipMemcpyAsync(h, S.head.p, sizeof(h), hipMemcpyDeviceToHost, st));
  FIESTA_HIP_CHECK(hipStreamSynchronize(st));
  if (h[TH_ERR_CONN]) throw Error(FIESTA_HIP_ERR_INVALID, "site_tour: two visited sites have no connection");
  if (h[TH_ERR_SYM]) throw Error(FIESTA_HIP_ERR_INVALID, "site_tour: the matrix is not symmetric among the visited sites");
  const int m = h[TH_M], max_moves = a.max_moves > 0 ? a.max_moves : 8 * m;
  if (m <= kTourLdsSites)
    hipLaunchKernelGGL(k_tour_search<true>, dim3(R), dim3(kTourThreads), 0, st, (const int32_t *)S.mat.p, m, closed, (unsigned long long)a.seed, max_moves,
                       S.tours.p, S.len.p, S.stat.p, S.head.p);
  else
    hipLaunchKernelGGL(k_tour_search<false>, dim3(R), dim3(kTourThreads), 0, st, (const int32_t *)S.mat.p, m, closed, (unsigned long long)a.seed, max_moves,
                       S.tours.p, S.len.p, S.stat.p, S.head.p);
  FIESTA_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_tour_pick, dim3(1), dim3(kTourThreads), 0, st, (const int32_t *)S.mat.p, m, n, closed, R, (const int32_t *)S.tours.p,
                     (const long long *)S.len.p, (const int32_t *)S.stat.p, (const int32_t *)S.site.p, (const int32_t *)S.status.p, S.head.p, dres);
  FIESTA_HIP_CHECK(hipGetLastError());
  if (a.info) FIESTA_HIP_CHECK(hipMemcpyAsync(a.info, S.head.p + TH_INFO, sizeof(fiesta_hip_tour_info), hipMemcpyDeviceToHost, st));
  if (!a.dev) out.back(order, n), out.back(site_status, n), out.back(leg_cost, n), out.back(restart_length, R);
  FIESTA_HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace
}  // namespace fiesta
