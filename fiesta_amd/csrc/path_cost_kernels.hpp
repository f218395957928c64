// fiesta_amd/csrc/path_cost_kernels.hpp -- batched path cost and waypoint gradients: fiesta_hip_path_cost / _dev (include/fiesta_hip.h).
//
// A trajectory optimiser holds thousands of candidate polylines and, per iteration, needs a smooth obstacle cost per polyline and the
// derivative of that cost with respect to every waypoint.  Through the point queries that is value + gradient of every sample moved
// to the caller (>= 32 B per sample), then the penalty, the chain rule and two scatter reductions on the caller's side.  Here the
// samples are path clearance's (path_kernels.hpp: same rule, same indices, the same evaluators, so a sample's (d, grad d) is the point
// query's bit for bit) and they are reduced on chip; per waypoint three words leave the device, per path four.
//   k_path_check / k_path_plan / k_path_pieces   path_kernels.hpp, unchanged
//   k_cost_eval      persistent grid, one wave per piece, lanes on consecutive samples as k_path_eval; every lane evaluates value AND
//                    gradient once.  A segment's sample 0 and the path's final sample are the waypoints themselves: their (phi, gamma)
//                    go straight to a per-waypoint record, one sample per waypoint, no reduction.  Interior samples feed seven sums
//                    per segment (sum phi, sum (1-t) gamma, sum t gamma).  The segment keys are non-decreasing across the lanes of a
//                    group, so the sums are a SEGMENTED WAVE SCAN (__shfl_up, the key compared at every step), the last lane of each
//                    run holds its total; the run that reaches lane 63 is carried into the next group in registers.  A run that ends
//                    inside the piece is stored by its last lane -- except the piece's first and last segment, which may be shared
//                    with the neighbouring pieces: those become the piece's head / tail record
//   k_cost_segments  one lane per head / tail record that starts a chain: the records of one segment are adjacent in piece order and
//                    are added in that order into the segment's sums (a segment of up to 2^24 samples spans many pieces)
//   k_cost_finish    one wave per path: lanes on consecutive segments, each computes its segment's cost term and its two
//                    contributions to the gradient (the one for its end waypoint travels one lane up); cost and length are added in
//                    segment order, n_below over the pieces
// No floating-point atomics, no scratch, no dependent global loads inside the sample loop.  Every sum has an order fixed by the
// call's arguments (the piece size follows n_paths): nothing depends on the grid size or on scheduling.
#pragma once
#include "path_kernels.hpp"

namespace fiesta {
namespace {  // (planner.hip alone includes this header; the namespace is part of the kernels' symbol names)

constexpr int kCostSegBlocks = 512;  // grid of k_cost_segments (a grid-stride loop over the piece records)

struct CostRec {  // one piece: the sums of its first segment (hk) and of its last one (tk; -1 if the piece lies in one segment)
  long long hk, tk, nb;  // nb: samples of the piece below the margin
  double h[7], t[7];
};

// ---- the per-term formulas (include/fiesta_hip.h), shared by the kernels and the host loop: fixed operation order ---------------
// phi and gamma = psi * grad of one sample; returns 1 if the sample counts for n_below
__host__ __device__ inline int cost_penalty(double v, const double *g, double margin, double *phi, double *gam) {
  if (v < margin) {
    const double e = margin - v;
    const double psi = -2.0 * e;
    *phi = e * e;
    gam[0] = psi * g[0], gam[1] = psi * g[1], gam[2] = psi * g[2];
    return 1;
  }
  *phi = 0, gam[0] = gam[1] = gam[2] = 0;
  return 0;
}
// the seven terms of interior sample k of S: phi, (1 - t) gamma, t gamma
__host__ __device__ inline void cost_terms(double phi, const double *gam, long long k, long long S, double *x) {
  const double t = (double)k / (double)S;
  const double r = 1.0 - t;
  x[0] = phi;
  x[1] = r * gam[0], x[2] = r * gam[1], x[3] = r * gam[2];
  x[4] = t * gam[0], x[5] = t * gam[1], x[6] = t * gam[2];
}
// Segment a -> b of S samples: ra / rb the waypoint records (phi, gamma) of its ends, s its seven sums.  *L its length, *hq its cost
// term h * Q, N / E its contributions to the gradients of a and of b.  L = 0: nothing but L.
__host__ __device__ inline void cost_segment(const double *a, const double *b, long long S, const double *ra, const double *rb, const double *s,
                                             double *L, double *hq, double *N, double *E) {
  const double d0 = b[0] - a[0], d1 = b[1] - a[1], d2 = b[2] - a[2];
  const double len = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
  *L = len;
  *hq = 0, N[0] = N[1] = N[2] = 0, E[0] = E[1] = E[2] = 0;
  if (!(len > 0)) return;
  const double Sd = (double)S;
  const double h = len / Sd;
  const double Q = (ra[0] * 0.5 + s[0]) + rb[0] * 0.5;
  const double qs = Q / Sd;
  const double d[3] = {d0, d1, d2};
  *hq = h * Q;
  for (int c = 0; c < 3; ++c) {
    const double u = d[c] / len;
    N[c] = h * (ra[1 + c] * 0.5 + s[1 + c]) - qs * u;
    E[c] = h * (s[4 + c] + rb[1 + c] * 0.5) + qs * u;
  }
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------------
template <class Eval>
__global__ __launch_bounds__(256) void k_cost_eval(Eval ev, const double *w, const int64_t *rng, const int64_t *base, const int64_t *nsamp,
                                                   const int64_t *poff, int64_t n_paths, long long max_pieces, double margin, double *wrec,
                                                   double *seg, CostRec *rec) {
  const int lane = threadIdx.x & 63;
  const int64_t total = poff[n_paths];
  const int64_t stride = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t piece = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6; piece < total; piece += stride) {
    const int64_t p = path_find(poff, 0, n_paths - 1, piece);
    const long long n = nsamp[p], ps = path_piece_size(n, max_pieces);
    const long long s0 = (piece - poff[p]) * ps, s1 = s0 + ps < n ? s0 + ps : n;
    const int64_t o0 = rng[2 * p], nw = rng[2 * p + 1] - o0;
    const double *pw = w + 3 * o0;
    const int64_t *pb = base + o0;
    int64_t jw = path_find(pb, 0, nw - 1, s0);  // the segment of the group's first sample (uniform in the wave)
    const long long jfirst = jw;                // the piece's first segment: its sums are the head record
    long long ck = -1;                          // the segment carried from the previous group (uniform), and its sums so far
    double cs[7] = {0, 0, 0, 0, 0, 0, 0};
    long long nb = 0;
    CostRec *out = rec + piece;
    for (long long sg = s0; sg < s1; sg += 64) {  // (every lane takes part in the shuffles, also past s1)
      const long long s = sg + lane;
      const long long bl = jw + lane < nw ? pb[jw + lane] : LLONG_MAX;  // first samples of segments jw .. jw + 63
      const long long bn = jw + 64 < nw ? pb[jw + 64] : LLONG_MAX;
      int i = 0;
      for (int h = 32; h > 0; h >>= 1) {
        const long long bm = __shfl(bl, i + h, 64);
        if (bm <= s) i += h;
      }
      const long long bj = __shfl(bl, i, 64), nx = __shfl(bl, i < 63 ? i + 1 : 63, 64);
      const long long end = i < 63 ? nx : bn;
      const int64_t j = jw + i;
      double x[7] = {0, 0, 0, 0, 0, 0, 0};
      if (s < s1) {
        double q[3], g[3], phi, gam[3];
        const double *a = pw + 3 * j;
        const long long k = s - bj;
        const bool waypoint = j == nw - 1 || k == 0;  // the final sample, or sample 0 of segment j: waypoint j itself
        if (j == nw - 1)
          q[0] = a[0], q[1] = a[1], q[2] = a[2];
        else
          path_point(a, k, end - bj, q);
        const double v = ev(q, g);
        nb += cost_penalty(v, g, margin, &phi, gam);
        if (waypoint) {
          double *r = wrec + 4 * (o0 + j);
          r[0] = phi, r[1] = gam[0], r[2] = gam[1], r[3] = gam[2];
        } else {
          cost_terms(phi, gam, k, end - bj, x);
        }
      }
      // lanes past the piece's end join the last sample's run with zeros
      const long long rest = s1 - 1 - sg;
      const long long jl = __shfl((long long)j, rest < 63 ? (int)rest : 63, 64);
      const long long key = s < s1 ? (long long)j : jl;
      for (int o = 1; o < 64; o <<= 1) {  // segmented inclusive scan: keys are non-decreasing, an equal key o lanes down means one run
        const long long ku = __shfl_up(key, o, 64);
        const bool same = lane >= o && ku == key;
#pragma unroll
        for (int c = 0; c < 7; ++c) {
          const double u = __shfl_up(x[c], o, 64);
          if (same) x[c] += u;
        }
      }
      const long long k0 = __shfl(key, 0, 64), k63 = __shfl(key, 63, 64), kn = __shfl_down(key, 1, 64);
      if (ck >= 0 && ck != k0 && lane == 0) {  // the carried segment ended with the previous group
        double *dst = ck == jfirst ? out->h : seg + 7 * (o0 + ck);
#pragma unroll
        for (int c = 0; c < 7; ++c) dst[c] = cs[c];
      }
      if (key == ck) {
#pragma unroll
        for (int c = 0; c < 7; ++c) x[c] = cs[c] + x[c];
      }
      if (lane < 63 && kn != key) {  // the last lane of a run that ends inside this group (key < k63)
        double *dst = key == jfirst ? out->h : seg + 7 * (o0 + key);
#pragma unroll
        for (int c = 0; c < 7; ++c) dst[c] = x[c];
      }
      ck = k63;
#pragma unroll
      for (int c = 0; c < 7; ++c) cs[c] = __shfl(x[c], 63, 64);
      jw = (int64_t)__shfl((long long)j, 63, 64) + (sg + 64 >= __shfl(end, 63, 64) ? 1 : 0);
    }
    nb = wave_sum(nb);
    if (lane == 0) {  // the piece's last segment: the tail record, or still the head
      double *dst = ck == jfirst ? out->h : out->t;
#pragma unroll
      for (int c = 0; c < 7; ++c) dst[c] = cs[c];
      out->hk = jfirst, out->tk = ck == jfirst ? -1 : ck, out->nb = nb;
    }
  }
}

// The head / tail records of a path in piece order: h_0 t_0 h_1 t_1 ...; records of one segment are adjacent (empty tails skipped).
// A tail always starts a chain (its key differs from its own head's); a head does if the piece before it ended on another segment.
__global__ __launch_bounds__(256) void k_cost_segments(const int64_t *rng, const int64_t *poff, int64_t n_paths, const CostRec *rec, double *seg) {
  const int64_t total = poff[n_paths];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t slot = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; slot < 2 * total; slot += stride) {
    const int64_t piece = slot >> 1;
    const bool tail = slot & 1;
    const long long key = tail ? rec[piece].tk : rec[piece].hk;
    if (key < 0) continue;
    const int64_t p = path_find(poff, 0, n_paths - 1, piece);
    if (!tail && piece > poff[p]) {
      const long long pt = rec[piece - 1].tk;
      if ((pt >= 0 ? pt : rec[piece - 1].hk) == key) continue;  // the chain started earlier
    }
    double sum[7];
    const double *src = tail ? rec[piece].t : rec[piece].h;
    for (int c = 0; c < 7; ++c) sum[c] = src[c];
    int64_t q = piece;
    bool at_tail = tail;
    for (;;) {  // the next record of the path, while it belongs to the same segment
      if (!at_tail && rec[q].tk >= 0) break;
      if (q + 1 >= poff[p + 1] || rec[q + 1].hk != key) break;
      ++q, at_tail = false;
      for (int c = 0; c < 7; ++c) sum[c] += rec[q].h[c];
    }
    double *dst = seg + 7 * (rng[2 * p] + key);
    for (int c = 0; c < 7; ++c) dst[c] = sum[c];
  }
}

__global__ __launch_bounds__(256) void k_cost_finish(const double *w, const int64_t *rng, const int64_t *base, const int64_t *nsamp,
                                                     const int64_t *poff, const double *wrec, const double *seg, const CostRec *rec,
                                                     int64_t n_paths, fiesta_hip_path_cost_result r) {
  const int64_t p = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (p >= n_paths) return;  // (uniform in the wave)
  const long long n = nsamp[p];
  if (n < 0) {  // invalid: its gradient rows (if its range is known at all) stay 0
    if (lane == 0) {
      if (r.cost) r.cost[p] = NAN;
      if (r.length) r.length[p] = NAN;
      if (r.n_below) r.n_below[p] = -1;
      if (r.n_samples) r.n_samples[p] = -1;
    }
    return;
  }
  const int64_t o0 = n > 0 ? rng[2 * p] : 0, nw = n > 0 ? rng[2 * p + 1] - o0 : 0;
  long long nb = 0;
  if (n > 0)
    for (int64_t k = poff[p] + lane; k < poff[p + 1]; k += 64) nb += rec[k].nb;
  nb = wave_sum(nb);
  double cost = 0, length = 0;     // (uniform: every lane adds the same terms in segment order)
  double ce[3] = {0, 0, 0};        // the contribution of the previous chunk's last segment to this chunk's first waypoint
  for (int64_t c = 0; c < nw; c += 64) {
    const int64_t j = c + lane;
    double L = 0, hq = 0, N[3] = {0, 0, 0}, E[3] = {0, 0, 0};
    if (j + 1 < nw) cost_segment(w + 3 * (o0 + j), w + 3 * (o0 + j + 1), base[o0 + j + 1] - base[o0 + j], wrec + 4 * (o0 + j), wrec + 4 * (o0 + j + 1),
                                 seg + 7 * (o0 + j), &L, &hq, N, E);
    for (int k = 0; k < 3; ++k) {
      const double up = __shfl_up(E[k], 1, 64);
      const double prev = lane == 0 ? ce[k] : up;  // E of segment j - 1 (0 before the path's first waypoint)
      ce[k] = __shfl(E[k], 63, 64);
      if (j < nw && r.grad) r.grad[3 * (o0 + j) + k] = N[k] + prev;
    }
    const int cnt = nw - 1 - c < 64 ? (int)(nw - 1 - c) : 64;
    for (int i = 0; i < cnt; ++i) {
      cost += __shfl(hq, i, 64);
      length += __shfl(L, i, 64);
    }
  }
  if (lane == 0) {
    if (r.cost) r.cost[p] = cost;
    if (r.length) r.length[p] = length;
    if (r.n_below) r.n_below[p] = nb;
    if (r.n_samples) r.n_samples[p] = n;
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
// The whole call on the host, sample by sample, every sum in sample / segment order (small batches: the brick cache).
template <class Eval>
void path_cost_host(Eval &ev, const double *w, int64_t n_wp, const int64_t *off, int64_t n_paths, double step, double margin,
                    const fiesta_hip_path_cost_result &r) {
  if (r.grad) std::fill(r.grad, r.grad + 3 * n_wp, 0.0);
  std::vector<long long> S;
  std::vector<double> rec, sums;
  for (int64_t p = 0; p < n_paths; ++p) {
    const int64_t o0 = off[p], nw = off[p + 1] - o0;
    const double *pw = w + 3 * o0;
    S.assign((size_t)std::max<int64_t>(nw, 1), 0);
    long long n = 0;
    bool bad = false;
    for (int64_t j = 0; j < nw; ++j) {
      if (!path_finite(pw + 3 * j) || (j + 1 < nw && !path_segment_samples(pw + 3 * j, pw + 3 * j + 3, step, &S[j]))) bad = true;
      n += S[j];
    }
    if (bad) {
      if (r.cost) r.cost[p] = NAN;
      if (r.length) r.length[p] = NAN;
      if (r.n_below) r.n_below[p] = -1;
      if (r.n_samples) r.n_samples[p] = -1;
      continue;
    }
    n = nw > 0 ? n + 1 : 0;
    rec.assign((size_t)std::max<int64_t>(nw, 1) * 4, 0.0);
    sums.assign((size_t)std::max<int64_t>(nw, 1) * 7, 0.0);
    long long nb = 0;
    for (int64_t j = 0; j < nw; ++j) {
      const long long Sj = j + 1 < nw ? S[j] : 1;
      for (long long k = 0; k < Sj; ++k) {
        double q[3], g[3], phi, gam[3], x[7];
        if (j + 1 < nw)
          path_point(pw + 3 * j, k, Sj, q);
        else
          q[0] = pw[3 * j], q[1] = pw[3 * j + 1], q[2] = pw[3 * j + 2];
        const double v = ev(q, g);
        nb += cost_penalty(v, g, margin, &phi, gam);
        if (k == 0) {
          rec[4 * j] = phi, rec[4 * j + 1] = gam[0], rec[4 * j + 2] = gam[1], rec[4 * j + 3] = gam[2];
        } else {
          cost_terms(phi, gam, k, Sj, x);
          for (int c = 0; c < 7; ++c) sums[7 * j + c] += x[c];
        }
      }
    }
    double cost = 0, length = 0, prev[3] = {0, 0, 0};
    for (int64_t j = 0; j < nw; ++j) {
      double L = 0, hq = 0, N[3] = {0, 0, 0}, E[3] = {0, 0, 0};
      if (j + 1 < nw) {
        cost_segment(pw + 3 * j, pw + 3 * j + 3, S[j], &rec[4 * j], &rec[4 * j + 4], &sums[7 * j], &L, &hq, N, E);
        cost += hq, length += L;
      }
      for (int c = 0; c < 3; ++c) {
        if (r.grad) r.grad[3 * (o0 + j) + c] = N[c] + prev[c];
        prev[c] = E[c];
      }
    }
    if (r.cost) r.cost[p] = cost;
    if (r.length) r.length[p] = length;
    if (r.n_below) r.n_below[p] = nb;
    if (r.n_samples) r.n_samples[p] = n;
  }
}

// The device pipeline.  w / off / r are device pointers; tmp is the map's grow-only scratch.  Nothing is read back.
template <class Eval>
void path_cost_launch(hipStream_t st, DevBuf<unsigned char> &tmp, const Eval &ev, const double *w, int64_t n_wp, const int64_t *off,
                      int64_t n_paths, double step, double margin, bool checked, const fiesta_hip_path_cost_result &r) {
  const long long max_pieces = std::max<int64_t>(1, kPathRecords / n_paths);
  const int64_t nrec = n_paths * max_pieces;  // <= max(kPathRecords, n_paths)
  const size_t b_nsamp = (size_t)n_wp * 8, b_rng = b_nsamp + (size_t)n_paths * 8, b_poff = b_rng + (size_t)n_paths * 16,
               b_wrec = b_poff + (size_t)(n_paths + 1) * 8, b_seg = b_wrec + (size_t)n_wp * 32, b_rec = b_seg + (size_t)n_wp * 56,
               bytes = b_rec + (size_t)nrec * sizeof(CostRec);
  tmp.ensure(bytes, st);
  int64_t *base = (int64_t *)tmp.p, *nsamp = (int64_t *)(tmp.p + b_nsamp), *rng = (int64_t *)(tmp.p + b_rng), *poff = (int64_t *)(tmp.p + b_poff);
  double *wrec = (double *)(tmp.p + b_wrec), *seg = (double *)(tmp.p + b_seg);
  CostRec *rec = (CostRec *)(tmp.p + b_rec);
  // rows of waypoints that belong to no valid path (gaps of a device batch's offsets, flagged paths) stay 0
  if (r.grad && n_wp > 0) FIESTA_HIP_CHECK(hipMemsetAsync(r.grad, 0, (size_t)n_wp * 24, st));
  if (checked) hipLaunchKernelGGL(k_path_check, dim3(1), dim3(1024), 0, st, off, n_paths, n_wp, nsamp, rng);
  hipLaunchKernelGGL(k_path_plan, dim3((unsigned)((n_paths + 3) / 4)), dim3(256), 0, st, w, off, n_paths, step, checked ? 1 : 0, base, nsamp,
                     rng);
  hipLaunchKernelGGL(k_path_pieces, dim3(1), dim3(1024), 0, st, (const int64_t *)nsamp, n_paths, max_pieces, poff);
  hipLaunchKernelGGL(k_cost_eval<Eval>, dim3(kPathEvalBlocks), dim3(256), 0, st, ev, w, (const int64_t *)rng, (const int64_t *)base,
                     (const int64_t *)nsamp, (const int64_t *)poff, n_paths, max_pieces, margin, wrec, seg, rec);
  hipLaunchKernelGGL(k_cost_segments, dim3(kCostSegBlocks), dim3(256), 0, st, (const int64_t *)rng, (const int64_t *)poff, n_paths,
                     (const CostRec *)rec, seg);
  hipLaunchKernelGGL(k_cost_finish, dim3((unsigned)((n_paths + 3) / 4)), dim3(256), 0, st, w, (const int64_t *)rng, (const int64_t *)base,
                     (const int64_t *)nsamp, (const int64_t *)poff, (const double *)wrec, (const double *)seg, (const CostRec *)rec, n_paths, r);
  FIESTA_HIP_CHECK(hipGetLastError());
}

// Both variants of the call on a map's stream, as path_clearance_run.
template <class Eval>
void path_cost_run(hipStream_t st, PlannerScratch &S, const Eval &ev, const PathCostArgs &a) {
  const fiesta_hip_path_cost_result &r = *a.res;
  if (a.dev) {
    path_cost_launch(st, S.tmp, ev, a.w, a.n_wp, a.off, a.n_paths, a.step, a.margin, true, r);
    return;
  }
  const size_t n = (size_t)a.n_paths, nw3 = (size_t)a.n_wp * 3;
  Staging in{S.in, st}, out{S.out, st};
  const auto w = in.add(a.w, nw3);
  const auto off = in.add(a.off, n + 1);
  in.alloc(), in.up(w, nw3), in.up(off, n + 1);
  const auto cost = out.add(r.cost, n), length = out.add(r.length, n), grad = out.add(r.grad, nw3);
  const auto n_below = out.add(r.n_below, n), n_samples = out.add(r.n_samples, n);
  out.alloc();
  const fiesta_hip_path_cost_result d{out.dev(cost), out.dev(grad), out.dev(length), out.dev(n_below), out.dev(n_samples)};
  path_cost_launch(st, S.tmp, ev, in.dev(w), a.n_wp, in.dev(off), a.n_paths, a.step, a.margin, false, d);
  out.back(cost, n), out.back(length, n), out.back(n_below, n), out.back(n_samples, n), out.back(grad, nw3);
  FIESTA_HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace
}  // namespace fiesta
