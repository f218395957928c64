// fiesta_amd/csrc/timing_kernels.hpp -- path timing: fiesta_hip_path_timing / _dev (include/fiesta_hip.h).
//
// How long a polyline takes: per sample of path clearance's sample rule a squared-speed limit from the clearance there (the speed
// from which the robot still stops within its free distance), a junction-deviation limit at the bends, rest (or v_start / v_end) at
// the ends, and the largest profile under those limits and the acceleration bound -- two prefix minima, a (min, +) recurrence
// written as a scan -- then the travel time of every interval.  Through the calls that existed this is every sample's value moved
// to the caller and a serial loop per path there.  Here a path is owned by one team of lanes and its whole computation runs inside
// ONE launch; per path seven words leave the device, per waypoint two.
//   k_path_check   path_kernels.hpp, unchanged (device variant only): offsets against the CSR rules
//   k_timing<Eval, TEAM, CAPS>  one team of TEAM lanes per path.  Instantiated twice:
//                    TEAM 64  (a one-wave work-group)  paths of at most kTimingWaveMax samples, the empty ones, those k_path_check
//                             flagged and those with more than FIESTA_HIP_TIMING_MAX_WAYPOINTS waypoints
//                    TEAM 256 (a four-wave work-group) the longer ones, up to FIESTA_HIP_TIMING_MAX_SAMPLES, and beyond (TOO_LONG)
//                  Both grids hold one work-group per path; both teams count the path's samples (S per segment by the sample rule,
//                  lanes on consecutive segments; W and the first sample index of every segment added in segment order by one lane:
//                  W's bits are ruled) and the team of the other class leaves: the class is chosen on the device, nothing is read back.
//                  count + validate -> [sample k: its segment by a binary search over the first-sample indices in LDS, the point
//                  query's value, the clearance limit, at a segment's sample 0 the corner limit, at both ends the end limit; lq and
//                  the segment index stay in LDS] -> forward scan of lq - P (the carry across trips in a register; f and P of a
//                  lane's samples stay in registers, the trips are unrolled) -> backward scan of lq + P, q = min(lq, f, b), v =
//                  sqrt(q) over lq in LDS -> [sample k: dt of the interval that ends at it, a team scan of dt gives its time; the
//                  samples that are waypoints write time and speed] -> team reductions for n_below, min_speed, min_index -> outputs
// min is exact and associative: the scans' shape does not show in any bit.  Only duration and time are sums with a free order,
// fixed by the path's sample count alone.  Every barrier sits in uniform control flow (branch decisions go through
// readfirstlane), every loop is bounded by the caps.  No atomics, no cooperative launch, no team waits for another.
#pragma once
#include "refine_kernels.hpp"

namespace fiesta {
namespace {  // (planner.hip alone includes this header; the namespace is part of the kernels' symbol names)

constexpr int kTimingWaveMax = 256;  // paths of at most this many samples are timed by one wave (four samples per lane)

struct TimingK {  // fiesta_hip_timing_params as the kernel uses it
  double step, margin, A, Vq, Mq, a_max, a_dev, vs2, ve2;  // A = 2 a_max, a_dev = a_max * corner_dev, vs2 / ve2 = v_start^2 / v_end^2
  int corner;                                              // corner_dev is finite
};

// ---- the per-term formulas (include/fiesta_hip.h): fixed operation order ---------------------------------------------------------
// the clearance limit of a sample of value d; *below: it counts for n_below
__host__ __device__ inline double timing_clearance_limit(double d, double margin, double A, double Vq, double Mq, int *below) {
  *below = d < margin ? 1 : 0;
  if (d < margin) return Mq;
  const double e = d - margin;
  double lq = A * e;
  if (lq > Vq) lq = Vq;
  if (lq < Mq) lq = Mq;
  return lq;
}
// the corner limit at the waypoint between the segments p -> a (length L0) and a -> b (length L1), both > 0; false: no limit
__host__ __device__ inline bool timing_corner_limit(const double *p, const double *a, const double *b, double L0, double L1, double a_dev,
                                                    double *cq) {
  double c = 0;
  {
    const double u0 = (a[0] - p[0]) / L0, u1 = (a[1] - p[1]) / L0, u2 = (a[2] - p[2]) / L0;
    const double w0 = (b[0] - a[0]) / L1, w1 = (b[1] - a[1]) / L1, w2 = (b[2] - a[2]) / L1;
    c = (u0 * w0 + u1 * w1) + u2 * w2;
  }
  if (c > 1.0) c = 1.0;
  if (c < -1.0) c = -1.0;
  const double sh = sqrt(0.5 * (1.0 + c));
  const double den = 1.0 - sh;
  if (!(den > 0)) return false;
  *cq = (a_dev * sh) / den;
  return true;
}
// the travel time of an interval of length h between the speeds v0 and v1
__host__ __device__ inline double timing_interval(double h, double v0, double v1, double a_max) {
  if (h == 0) return 0.0;
  const double sv = v0 + v1;
  if (sv > 0) return (2.0 * h) / sv;
  return 2.0 * sqrt(h / a_max);
}
// the last j in [0, hi] with base[j] <= s (base[0] = 0 <= s)
__device__ inline int timing_find(const int *base, int hi, int s) {
  int lo = 0;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (base[mid] <= s)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

// Inclusive scan of one value per lane over the team, in thread order (REV: in reverse thread order, a suffix scan); *total = the
// whole team's, the same bits in every lane.  lds: one word per wave; a team of several waves holds two barriers, the second frees
// lds for the next call.  Called by every lane of the team, in uniform control flow.
template <int TEAM, bool REV, class Op>
__device__ inline double timing_scan(double v, double ident, Op op, double *lds, double *total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (REV) v = __shfl(v, 63 - lane, 64);
  v = wave_inclusive(v, op);  // (lane 63 holds the wave's)
  if (TEAM > 64) {
    if (lane == 63) lds[wv] = v;
    __syncthreads();
    double pre = ident, tot = ident;
    for (int k = 0; k < TEAM / 64; ++k) {
      if (REV ? k > wv : k < wv) pre = op(pre, lds[k]);
      tot = op(tot, lds[k]);
    }
    __syncthreads();
    v = op(pre, v);
    *total = tot;
  } else {
    *total = __shfl(v, 63, 64);
  }
  return REV ? __shfl(v, 63 - lane, 64) : v;
}

// the outputs of a path that is not timed (status != OK), or of an empty one
__device__ inline void timing_write_none(const fiesta_hip_path_timing_result &r, int64_t p, int status) {
  const bool ok = status == FIESTA_HIP_TIMING_OK;
  const double nan = NAN;
  if (r.duration) r.duration[p] = ok ? 0.0 : nan;
  if (r.length) r.length[p] = ok ? 0.0 : nan;
  if (r.n_samples) r.n_samples[p] = ok ? 0 : -1;
  if (r.n_below) r.n_below[p] = ok ? 0 : -1;
  if (r.min_speed) r.min_speed[p] = ok ? (double)INFINITY : nan;
  if (r.min_index) r.min_index[p] = -1;
  if (r.status) r.status[p] = status;
}

template <class Eval, int TEAM, int CAPS>
__global__ __launch_bounds__(TEAM) void k_timing(Eval ev, const double *w, const int64_t *off, const int64_t *nsamp, const int64_t *rng,
                                                 int checked, int64_t n_paths, TimingK k, fiesta_hip_path_timing_result r) {
  constexpr int CAPW = CAPS < FIESTA_HIP_TIMING_MAX_WAYPOINTS ? CAPS : FIESTA_HIP_TIMING_MAX_WAYPOINTS;  // (m <= n: S >= 1)
  constexpr int NT = CAPS / TEAM;  // trips of the scans
  __shared__ double lq[CAPS];          // per sample: lq, later v
  __shared__ unsigned short sg[CAPS];  // per sample: its segment
  __shared__ double Wl[CAPW], Ll[CAPW];  // per waypoint j: W_j; per segment j: L_j
  __shared__ int bs[CAPW];             // per waypoint: its sample (S_j until the serial pass)
  __shared__ double red[2][4];
  __shared__ int n_lds;
  const int t = threadIdx.x;
  refine_in_vgpr(k.margin), refine_in_vgpr(k.A), refine_in_vgpr(k.Vq), refine_in_vgpr(k.Mq), refine_in_vgpr(k.a_max), refine_in_vgpr(k.a_dev);
  refine_in_vgpr(k.vs2), refine_in_vgpr(k.ve2), refine_in_vgpr(k.step);
  refine_in_vgpr(r.duration), refine_in_vgpr(r.length), refine_in_vgpr(r.n_samples), refine_in_vgpr(r.n_below), refine_in_vgpr(r.min_speed);
  refine_in_vgpr(r.min_index), refine_in_vgpr(r.status), refine_in_vgpr(r.time), refine_in_vgpr(r.speed);
  int rb = 0;  // reductions so far (uniform): they alternate between the two rows of red
  const int64_t p = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
  if (p >= n_paths) return;
  const bool flagged = checked && nsamp[p] < 0;  // offsets out of order or out of range (k_path_check)
  int64_t o0 = flagged ? 0 : (checked ? rng[2 * p] : off[p]);
  const int64_t o1 = flagged ? 0 : (checked ? rng[2 * p + 1] : off[p + 1]);
  const int64_t len = o1 - o0;
  const bool many = len > FIESTA_HIP_TIMING_MAX_WAYPOINTS;
  // ---- the class, as far as the waypoint count says it (uniform in the team) ----
  if (TEAM == 64 ? !(flagged || many || len <= kTimingWaveMax) : (flagged || many)) return;
  if (flagged || many || len == 0) {  // (the wave team only)
    if (t == 0) timing_write_none(r, p, flagged ? FIESTA_HIP_TIMING_INVALID : (many ? FIESTA_HIP_TIMING_TOO_LONG : FIESTA_HIP_TIMING_OK));
    return;
  }
  const int m = (int)len;  // 1 .. CAPW
  const double *pw = w + 3 * o0;
  refine_in_vgpr(pw), refine_in_vgpr(o0);
  // ---- count: L and S per segment, validate; then W and the first sample of every segment, in segment order ----
  {
    double lane_bad = 0.0;
    for (int j = t; j < m; j += TEAM) {
      const double *a = pw + 3 * j;
      if (!path_finite(a)) lane_bad = 1.0;
      long long S = 0;
      double L = 0;
      if (j + 1 < m) {
        if (!path_segment_samples(a, a + 3, k.step, &S)) lane_bad = 1.0, S = 0;
        const double d0 = a[3] - a[0], d1 = a[4] - a[1], d2 = a[5] - a[2];
        L = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
      }
      Ll[j] = L;
      bs[j] = S > FIESTA_HIP_TIMING_MAX_SAMPLES ? FIESTA_HIP_TIMING_MAX_SAMPLES + 1 : (int)S;
    }
    const bool bad = __builtin_amdgcn_readfirstlane(refine_reduce<TEAM>(lane_bad, red[rb++ & 1], WaveMax{}) > 0.0 ? 1 : 0) != 0;
    if (bad) {  // its team: by the waypoint count alone
      if ((TEAM == 64) == (m <= kTimingWaveMax) && t == 0) timing_write_none(r, p, FIESTA_HIP_TIMING_INVALID);
      return;
    }
  }
  if (t == 0) {
    double W = 0;
    int at = 0;  // (saturates above the cap: n > MAX_SAMPLES is all that is asked of it then)
    for (int j = 0; j < m; ++j) {
      const int S = bs[j];
      Wl[j] = W, bs[j] = at;
      W = W + Ll[j];  // (L of the last waypoint is 0, its S is 0)
      at = at + S > FIESTA_HIP_TIMING_MAX_SAMPLES + 1 ? FIESTA_HIP_TIMING_MAX_SAMPLES + 1 : at + S;
    }
    n_lds = at + 1;
  }
  __syncthreads();
  const int n = __builtin_amdgcn_readfirstlane(n_lds);
  if ((TEAM == 64) != (n <= kTimingWaveMax)) return;  // the other class's path
  if (n > FIESTA_HIP_TIMING_MAX_SAMPLES || n > CAPS) {
    if (t == 0) timing_write_none(r, p, FIESTA_HIP_TIMING_TOO_LONG);
    return;
  }
  // ---- the samples: lq and the segment of every one ----
  double nb = 0.0;
  for (int s = t; s < n; s += TEAM) {
    const int j = timing_find(bs, m - 1, s);
    const double *a = pw + 3 * j;
    double q[3];
    if (j == m - 1)
      q[0] = a[0], q[1] = a[1], q[2] = a[2];  // the final sample: the last waypoint itself
    else
      path_point(a, s - bs[j], bs[j + 1] - bs[j], q);
    const double d = ev(q, nullptr);
    int below;
    double x = timing_clearance_limit(d, k.margin, k.A, k.Vq, k.Mq, &below);
    nb += (double)below;  // (at most 4096: exact)
    if (k.corner && s == bs[j] && j >= 1 && j <= m - 2) {
      const double L0 = Ll[j - 1], L1 = Ll[j];
      double cq;
      if (L0 > 0 && L1 > 0 && timing_corner_limit(a - 3, a, a + 3, L0, L1, k.a_dev, &cq) && cq < x) x = cq;
    }
    if (s == 0 && k.vs2 < x) x = k.vs2;
    if (s == n - 1 && k.ve2 < x) x = k.ve2;
    lq[s] = x, sg[s] = (unsigned short)j;
  }
  __syncthreads();  // (the scans read only what their own lane wrote; sg and lq of the neighbours are read further down)
  // ---- forward: f_k = min_{j <= k} (lq_j - P_j) + P_k; a lane's f and P stay in registers ----
  double fr[NT], Pr[NT];
  {
    double carry = INFINITY;
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      fr[i] = 0, Pr[i] = 0;
      if (i * TEAM < n) {  // (uniform)
        const int s = i * TEAM + t;
        double P = 0, x = INFINITY;
        if (s < n) {
          const int j = sg[s];
          const double arc = j == m - 1 ? Wl[j] : Wl[j] + Ll[j] * ((double)(s - bs[j]) / (double)(bs[j + 1] - bs[j]));
          P = k.A * arc;
          x = lq[s] - P;
        }
        double tot;
        double inc = timing_scan<TEAM, false>(x, (double)INFINITY, WaveMin{}, red[rb++ & 1], &tot);
        inc = carry < inc ? carry : inc;
        carry = tot < carry ? tot : carry;
        fr[i] = inc + P, Pr[i] = P;
      }
    }
  }
  // ---- backward: b_k = min_{j >= k} (lq_j + P_j) - P_k; q_k = min(lq_k, f_k, b_k); v_k = sqrt(q_k) replaces lq_k ----
  {
    double carry = INFINITY;
#pragma unroll
    for (int i = NT - 1; i >= 0; --i) {
      if (i * TEAM < n) {  // (uniform)
        const int s = i * TEAM + t;
        const double x = s < n ? lq[s] + Pr[i] : (double)INFINITY;
        double tot;
        double suf = timing_scan<TEAM, true>(x, (double)INFINITY, WaveMin{}, red[rb++ & 1], &tot);
        suf = carry < suf ? carry : suf;
        carry = tot < carry ? tot : carry;
        if (s < n) {
          const double b = suf - Pr[i];
          double q = lq[s];
          if (fr[i] < q) q = fr[i];
          if (b < q) q = b;
          lq[s] = sqrt(q);
        }
      }
    }
  }
  __syncthreads();
  // ---- intervals: sample s takes the interval that ends at it; the scan of dt is its time ----
  double tcarry = 0.0, vmin = INFINITY, imin = 0.0;
  for (int c = 0; c < n; c += TEAM) {  // (uniform)
    const int s = c + t;
    double dt = 0.0, v = 0.0;
    if (s < n) {
      v = lq[s];
      if (s > 0) {
        const int j = sg[s - 1];
        dt = timing_interval(Ll[j] / (double)(bs[j + 1] - bs[j]), lq[s - 1], v, k.a_max);
      }
      if (v < vmin) vmin = v, imin = (double)s;  // (a lane's samples ascend: a tie keeps the lower index)
    }
    double tot;
    const double at = tcarry + timing_scan<TEAM, false>(dt, 0.0, WaveSum{}, red[rb++ & 1], &tot);
    tcarry = tcarry + tot;
    if (s < n) {
      const int j = sg[s];
      if (s == bs[j]) {  // waypoint j itself
        if (r.time) r.time[o0 + j] = at;
        if (r.speed) r.speed[o0 + j] = v;
      }
    }
  }
  nb = refine_reduce<TEAM>(nb, red[rb++ & 1], WaveSum{});
  const double vm = refine_reduce<TEAM>(vmin, red[rb++ & 1], WaveMin{});
  const double im = refine_reduce<TEAM>(vmin == vm ? imin : (double)CAPS, red[rb++ & 1], WaveMin{});
  if (t == 0) {
    if (r.duration) r.duration[p] = tcarry;
    if (r.length) r.length[p] = Wl[m - 1];
    if (r.n_samples) r.n_samples[p] = n;
    if (r.n_below) r.n_below[p] = (int64_t)nb;
    if (r.min_speed) r.min_speed[p] = vm;
    if (r.min_index) r.min_index[p] = (int64_t)im;
    if (r.status) r.status[p] = FIESTA_HIP_TIMING_OK;
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
// The device pipeline.  w / off / r are device pointers; tmp is the map's grow-only scratch.  Nothing is read back.
template <class Eval>
void path_timing_launch(hipStream_t st, DevBuf<unsigned char> &tmp, const Eval &ev, const double *w, int64_t n_wp, const int64_t *off,
                        int64_t n_paths, const fiesta_hip_timing_params &par, bool checked, const fiesta_hip_path_timing_result &r) {
  tmp.ensure((size_t)n_paths * 24, st);
  int64_t *nsamp = (int64_t *)tmp.p, *rng = (int64_t *)(tmp.p + (size_t)n_paths * 8);
  // rows that belong to no timed path (gaps of a device batch's offsets, INVALID and TOO_LONG paths) are NaN (all bits set); a
  // timed path's team writes each of its rows once
  if (r.time && n_wp > 0) FIESTA_HIP_CHECK(hipMemsetAsync(r.time, 0xFF, (size_t)n_wp * 8, st));
  if (r.speed && n_wp > 0) FIESTA_HIP_CHECK(hipMemsetAsync(r.speed, 0xFF, (size_t)n_wp * 8, st));
  if (checked) hipLaunchKernelGGL(k_path_check, dim3(1), dim3(1024), 0, st, off, n_paths, n_wp, nsamp, rng);
  const bool corner = std::isfinite(par.corner_dev);
  const TimingK k{par.step,  par.margin, 2.0 * par.a_max, par.v_max * par.v_max, par.v_min * par.v_min,
                  par.a_max, corner ? par.a_max * par.corner_dev : 0.0, par.v_start * par.v_start, par.v_end * par.v_end, corner ? 1 : 0};
  const dim3 grid((unsigned)std::min<int64_t>(n_paths, kRefineGridX), (unsigned)((n_paths + kRefineGridX - 1) / kRefineGridX));
  hipLaunchKernelGGL((k_timing<Eval, 64, kTimingWaveMax>), grid, dim3(64), 0, st, ev, w, off, (const int64_t *)nsamp, (const int64_t *)rng,
                     checked ? 1 : 0, n_paths, k, r);
  hipLaunchKernelGGL((k_timing<Eval, 256, FIESTA_HIP_TIMING_MAX_SAMPLES>), grid, dim3(256), 0, st, ev, w, off, (const int64_t *)nsamp,
                     (const int64_t *)rng, checked ? 1 : 0, n_paths, k, r);
  FIESTA_HIP_CHECK(hipGetLastError());
}

// Both variants of the call on a map's stream, as path_refine_run.
template <class Eval>
void path_timing_run(hipStream_t st, PlannerScratch &S, const Eval &ev, const PathTimingArgs &a) {
  const fiesta_hip_path_timing_result &r = *a.res;
  if (a.dev) {
    path_timing_launch(st, S.tmp, ev, a.w, a.n_wp, a.off, a.n_paths, *a.par, true, r);
    return;
  }
  const size_t n = (size_t)a.n_paths, nw = (size_t)a.n_wp;
  Staging in{S.in, st}, out{S.out, st};
  const auto w = in.add(a.w, 3 * nw);
  const auto off = in.add(a.off, n + 1);
  in.alloc(), in.up(w, 3 * nw), in.up(off, n + 1);
  const auto duration = out.add(r.duration, n), length = out.add(r.length, n), min_speed = out.add(r.min_speed, n);
  const auto n_samples = out.add(r.n_samples, n), n_below = out.add(r.n_below, n), min_index = out.add(r.min_index, n);
  const auto status = out.add(r.status, n);
  const auto time = out.add(r.time, nw), speed = out.add(r.speed, nw);
  out.alloc();
  const fiesta_hip_path_timing_result d{out.dev(duration), out.dev(length), out.dev(n_samples), out.dev(n_below), out.dev(min_speed),
                                        out.dev(min_index), out.dev(status),  out.dev(time),      out.dev(speed)};
  path_timing_launch(st, S.tmp, ev, in.dev(w), a.n_wp, in.dev(off), a.n_paths, *a.par, false, d);
  out.back(duration, n), out.back(length, n), out.back(n_samples, n), out.back(n_below, n), out.back(min_speed, n), out.back(min_index, n);
  out.back(status, n), out.back(time, nw), out.back(speed, nw);
  FIESTA_HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace
}  // namespace fiesta
