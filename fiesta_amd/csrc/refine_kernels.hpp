// fiesta_amd/csrc/refine_kernels.hpp -- path refinement: fiesta_hip_path_refine / _dev (include/fiesta_hip.h).
//
// The optimiser's loop itself: every polyline of a CSR batch takes `iterations` projected-gradient steps on an obstacle cost (path
// cost's penalty at the waypoints) plus a smoothness cost (squared second differences), every waypoint clamped to a box of its own.
// Through the calls that existed this is, per iteration, a gradient query, a stencil, a step and a clamp from the host: tens of
// launches, and every path of the batch in lock-step.  Here the whole loop of a path runs inside ONE launch: the paths are
// independent, so a path is owned by one team of lanes, its positions stay in LDS across the iterations (two parities: the update is
// a Jacobi step), and nothing but the team's own barrier synchronises anything.
//   k_path_check   path_kernels.hpp, unchanged (device variant only): offsets against the CSR rules
//   k_refine<Eval, TEAM, CAP>  one team of TEAM lanes per path, lanes on consecutive waypoints (stride TEAM).  Instantiated twice:
//                    TEAM 64  (a one-wave work-group)  paths of at most kRefineWaveMax waypoints, and the paths k_path_check flagged
//                    TEAM 256 (a four-wave work-group) the longer ones, up to FIESTA_HIP_REFINE_MAX_WAYPOINTS (2 x 1024 x 3 f64 of
//                             LDS = 48 KB) and beyond (INVALID)
//                  Both grids hold one work-group per path; a team looks at its path's length and leaves the paths of the other class alone, so
//                  the class is chosen on the device and the _dev variant reads nothing back.
//                  load + validate -> [iteration: sample (d, grad d) at the waypoint by the point query's code, second differences
//                  of the five-point neighbourhood out of LDS, step, two clamps, write the other parity, team maximum of the move]
//                  -> one more pass over all waypoints for J, n_below and min_dist -> outputs.  (J at the input positions is
//                  gathered by the first pass, whichever kind it is.)
// The stop decision follows a team reduction whose result every lane of the team holds: no barrier sits in divergent code.  Every
// loop is bounded by `iterations` and the waypoint cap.  No atomics, no cooperative launch, no team waits for another.  The sums of J
// are added per lane in waypoint order (stride TEAM), then across lanes by a butterfly, then across waves in wave order: fixed by the
// path's length alone.
#pragma once
#include "path_cost_kernels.hpp"

namespace fiesta {
namespace {  // (planner.hip alone includes this header; the namespace is part of the kernels' symbol names)

constexpr int kRefineWaveMax = 128;        // paths of at most this many waypoints are refined by one wave (two waypoints per lane)
constexpr int64_t kRefineGridX = 1 << 15;  // work-groups per grid row: path p is work-group (p % 2^15, p / 2^15)
constexpr double kRefineMaxCoord = 1099511627776.0;  // 2^40

struct RefineK {  // fiesta_hip_refine_params as the kernel uses it
  double margin, wo, ws, ws2, alpha, max_step, tol;
  int iterations;
};

// v reduced over the team; every lane returns the same bits (op is commutative: both partners of a butterfly step compute the same
// value).  Holds exactly one barrier, which also orders the team's LDS writes before it against the reads after it.  red: TEAM / 64
// words that no reduction of the two before this one used.
template <int TEAM, class Op>
__device__ inline double refine_reduce(double v, double *red, Op op) {
  v = wave_reduce(v, op);
  if (TEAM > 64) {
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = red[0];
    for (int k = 1; k < TEAM / 64; ++k) v = op(v, red[k]);
  } else {
    __syncthreads();
  }
  return v;
}

// Keeps a wave-uniform value in a vector register from here on.  The sample code (Geom, the page table) fills the scalar file; the
// weights and the result's pointers are only ever operands of vector instructions, and vector registers are plentiful here.
template <class T>
__device__ inline void refine_in_vgpr(T &x) {
  asm volatile("" : "+v"(x));
}

// the second difference a_j[c] of positions w (x3) of a path of m waypoints: 0 at both ends
__device__ inline double refine_a(const double *w, int j, int m, int c) {
  if (j <= 0 || j >= m - 1) return 0.0;
  return (w[3 * (j - 1) + c] - 2.0 * w[3 * j + c]) + w[3 * (j + 1) + c];
}

template <class Eval, int TEAM, int CAP>
__global__ __launch_bounds__(TEAM) void k_refine(Eval ev, const double *w, const int64_t *off, const int64_t *nsamp, const int64_t *rng,
                                                 int checked, int64_t n_paths, const double *bounds, RefineK k, fiesta_hip_refine_result r) {
  __shared__ double pos[2][3 * CAP];
  __shared__ double red[2][4];
  const int t = threadIdx.x;
  refine_in_vgpr(k.margin), refine_in_vgpr(k.wo), refine_in_vgpr(k.ws), refine_in_vgpr(k.ws2), refine_in_vgpr(k.alpha), refine_in_vgpr(k.max_step);
  refine_in_vgpr(r.waypoints), refine_in_vgpr(r.cost), refine_in_vgpr(r.last_move), refine_in_vgpr(r.iterations), refine_in_vgpr(r.n_below);
  refine_in_vgpr(r.min_dist), refine_in_vgpr(r.status);
  int rb = 0;  // reductions so far (uniform): they alternate between the two rows of red
  {  // (one path per team, no loop over paths: what the prologue reads is dead before the passes start)
    const int64_t p = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (p >= n_paths) return;
    const bool flagged = checked && nsamp[p] < 0;  // offsets out of order or out of range (k_path_check)
    int64_t o0 = flagged ? 0 : (checked ? rng[2 * p] : off[p]);
    const int64_t o1 = flagged ? 0 : (checked ? rng[2 * p + 1] : off[p + 1]);
    const int64_t len = o1 - o0;
    const bool mine = TEAM == 64 ? (flagged || len <= kRefineWaveMax) : (!flagged && len > kRefineWaveMax);
    if (!mine) return;  // (uniform in the team)
    bool bad = flagged || len > FIESTA_HIP_REFINE_MAX_WAYPOINTS || len > CAP;
    const int m = bad ? 0 : (int)len;
    const double *pw = w + 3 * o0;
    const double *pb = bounds ? bounds + 6 * o0 : nullptr;
    const bool bounded = bounds != nullptr;
    refine_in_vgpr(pb), refine_in_vgpr(o0);
    if (!bad) {
      double lane_bad = 0.0;
      for (int j = t; j < m; j += TEAM) {
        for (int c = 0; c < 3; ++c) {
          const double x = pw[3 * j + c];
          if (!(fabs(x) <= kRefineMaxCoord)) lane_bad = 1.0;  // (a NaN fails the comparison)
          pos[0][3 * j + c] = x, pos[1][3 * j + c] = x;
        }
        if (bounded && j >= 1 && j <= m - 2)
          for (int c = 0; c < 3; ++c) {
            const double lo = pb[6 * j + c], hi = pb[6 * j + 3 + c];
            if (!(lo <= hi)) lane_bad = 1.0;  // lo > hi, or a NaN
          }
      }
      bad = __builtin_amdgcn_readfirstlane(refine_reduce<TEAM>(lane_bad, red[rb++ & 1], WaveMax{}) > 0.0 ? 1 : 0) != 0;
    }
    if (bad) {  // its rows keep the input (the row copy, or the caller's own array)
      if (t == 0) {
        const double nan = NAN;
        if (r.cost) r.cost[2 * p] = nan, r.cost[2 * p + 1] = nan;
        if (r.last_move) r.last_move[p] = nan;
        if (r.iterations) r.iterations[p] = -1;
        if (r.n_below) r.n_below[p] = -1;
        if (r.min_dist) r.min_dist[p] = nan;
        if (r.status) r.status[p] = FIESTA_HIP_REFINE_INVALID;
      }
      return;
    }
    // ---- the passes: read parity P, write the other one (both hold the ends, which never move).  Pass `it` is iteration it + 1,
    // or -- once the iterations are done or the path has stopped -- the final pass: J, n_below and min_dist at the final positions,
    // the latter two over the ends as well.  One loop serves both, so the sample code is instantiated once. ----
    int it = 0, P = 0;
    double last = 0.0, j0 = 0.0, j1 = 0.0, nb = 0.0, md = INFINITY;  // j0 / j1: this lane's terms of J at the input / final positions
    bool stop = m <= 2;
    for (;;) {
      const bool fin = stop || it >= k.iterations;  // (uniform in the team)
      const double *cur = pos[P];
      double *nxt = pos[P ^ 1];
      double mv = 0.0;
      for (int i = (fin ? 0 : 1) + t; i < (fin ? m : m - 1); i += TEAM) {
        double q[3] = {cur[3 * i], cur[3 * i + 1], cur[3 * i + 2]}, g[3], phi, gam[3], aa[3];
        const double d = ev(q, g);
        const int below = cost_penalty(d, g, k.margin, &phi, gam);
        for (int c = 0; c < 3; ++c) aa[c] = refine_a(cur, i, m, c);
        const double e = k.wo * phi + k.ws * ((aa[0] * aa[0] + aa[1] * aa[1]) + aa[2] * aa[2]);
        const bool inner = i >= 1 && i <= m - 2;
        if (it == 0 && inner) j0 += e;
        if (fin) {
          if (inner) j1 += e;
          nb += (double)below;  // (at most 1024: exact)
          md = d < md ? d : md;
          if (r.waypoints)
            for (int c = 0; c < 3; ++c) r.waypoints[3 * (o0 + i) + c] = q[c];
          continue;
        }
        for (int c = 0; c < 3; ++c) {
          const double s = (refine_a(cur, i - 1, m, c) - 2.0 * aa[c]) + refine_a(cur, i + 1, m, c);
          const double G = k.wo * gam[c] + k.ws2 * s;
          double delta = k.alpha * G;
          if (delta > k.max_step) delta = k.max_step;
          if (delta < -k.max_step) delta = -k.max_step;
          double x = q[c] - delta;
          if (bounded) {
            const double lo = pb[6 * i + c], hi = pb[6 * i + 3 + c];
            if (x < lo) x = lo;
            if (x > hi) x = hi;
          }
          const double move = fabs(x - q[c]);
          mv = move > mv ? move : mv;
          nxt[3 * i + c] = x;
        }
      }
      if (fin) break;
      last = refine_reduce<TEAM>(mv, red[rb++ & 1], WaveMax{});
      ++it, P ^= 1;
      stop = __builtin_amdgcn_readfirstlane(last <= k.tol ? 1 : 0) != 0;  // (every lane holds the team's maximum: a scalar branch)
    }
    j1 = refine_reduce<TEAM>(j1, red[rb++ & 1], WaveSum{});
    j0 = it > 0 ? refine_reduce<TEAM>(j0, red[rb++ & 1], WaveSum{}) : j1;  // (nothing ran: the input is the result)
    nb = refine_reduce<TEAM>(nb, red[rb++ & 1], WaveSum{});
    md = refine_reduce<TEAM>(md, red[rb++ & 1], WaveMin{});
    if (t == 0) {
      if (r.cost) r.cost[2 * p] = j0, r.cost[2 * p + 1] = j1;
      if (r.last_move) r.last_move[p] = last;
      if (r.iterations) r.iterations[p] = it;
      if (r.n_below) r.n_below[p] = (int64_t)nb;
      if (r.min_dist) r.min_dist[p] = md;
      if (r.status) r.status[p] = FIESTA_HIP_REFINE_OK;
    }
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
// The device pipeline.  w / off / bounds / r are device pointers; tmp is the map's grow-only scratch.  Nothing is read back.
template <class Eval>
void path_refine_launch(hipStream_t st, DevBuf<unsigned char> &tmp, const Eval &ev, const double *w, int64_t n_wp, const int64_t *off,
                        int64_t n_paths, const double *bounds, const fiesta_hip_refine_params &par, bool checked,
                        const fiesta_hip_refine_result &r) {
  tmp.ensure((size_t)n_paths * 24, st);
  int64_t *nsamp = (int64_t *)tmp.p, *rng = (int64_t *)(tmp.p + (size_t)n_paths * 8);
  // rows that belong to no valid path (gaps of a device batch's offsets, invalid paths) equal the input; a valid path's rows are
  // written by its team after it has read them all
  if (r.waypoints && r.waypoints != w && n_wp > 0)
    FIESTA_HIP_CHECK(hipMemcpyAsync(r.waypoints, w, (size_t)n_wp * 24, hipMemcpyDeviceToDevice, st));
  if (checked) hipLaunchKernelGGL(k_path_check, dim3(1), dim3(1024), 0, st, off, n_paths, n_wp, nsamp, rng);
  const RefineK k{par.margin, par.w_obstacle, par.w_smooth, 2.0 * par.w_smooth, par.alpha, par.max_step, par.tolerance, par.iterations};
  const dim3 grid((unsigned)std::min<int64_t>(n_paths, kRefineGridX), (unsigned)((n_paths + kRefineGridX - 1) / kRefineGridX));
  hipLaunchKernelGGL((k_refine<Eval, 64, kRefineWaveMax>), grid, dim3(64), 0, st, ev, w, off, (const int64_t *)nsamp, (const int64_t *)rng,
                     checked ? 1 : 0, n_paths, bounds, k, r);
  hipLaunchKernelGGL((k_refine<Eval, 256, FIESTA_HIP_REFINE_MAX_WAYPOINTS>), grid, dim3(256), 0, st, ev, w, off, (const int64_t *)nsamp,
                     (const int64_t *)rng, checked ? 1 : 0, n_paths, bounds, k, r);
  FIESTA_HIP_CHECK(hipGetLastError());
}

// Both variants of the call on a map's stream, as path_cost_run.
template <class Eval>
void path_refine_run(hipStream_t st, PlannerScratch &S, const Eval &ev, const PathRefineArgs &a) {
  const fiesta_hip_refine_result &r = *a.res;
  if (a.dev) {
    path_refine_launch(st, S.tmp, ev, a.w, a.n_wp, a.off, a.n_paths, a.bounds, *a.par, true, r);
    return;
  }
  const size_t n = (size_t)a.n_paths, nw3 = (size_t)a.n_wp * 3;
  Staging in{S.in, st}, out{S.out, st};
  const auto w = in.add(a.w, nw3);
  const auto off = in.add(a.off, n + 1);
  const auto bounds = in.add(a.bounds, 2 * nw3);
  in.alloc(), in.up(w, nw3), in.up(off, n + 1), in.up(bounds, 2 * nw3);
  const auto wp = out.add(r.waypoints, nw3), cost = out.add(r.cost, 2 * n), last_move = out.add(r.last_move, n), min_dist = out.add(r.min_dist, n);
  const auto iterations = out.add(r.iterations, n), status = out.add(r.status, n);
  const auto n_below = out.add(r.n_below, n);
  out.alloc();
  const fiesta_hip_refine_result d{out.dev(wp),      out.dev(cost),     out.dev(last_move), out.dev(iterations),
                                   out.dev(n_below), out.dev(min_dist), out.dev(status)};
  path_refine_launch(st, S.tmp, ev, in.dev(w), a.n_wp, in.dev(off), a.n_paths, in.dev(bounds), *a.par, false, d);
  out.back(wp, nw3), out.back(cost, 2 * n), out.back(last_move, n), out.back(iterations, n), out.back(n_below, n), out.back(min_dist, n);
  out.back(status, n);
  FIESTA_HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace
}  // namespace fiesta
