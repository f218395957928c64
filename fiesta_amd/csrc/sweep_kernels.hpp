// fiesta_amd/csrc/sweep_kernels.hpp -- body sweeps: a sphere-set body checked along batched pose polylines: fiesta_hip_body_sweep / _dev
// (include/fiesta_hip.h).
//
// A sampling planner asks of every edge it tries whether the MOTION is free for the BODY.  Through the body call that is: build every
// intermediate pose, upload 56 B per sample, query them all, then a segmented minimum, arg-minimum and first-below per edge on the
// caller's side.  Here the poses between two waypoint poses are generated on chip by the header's rule (positions: the path rule;
// rotations: normalised linear interpolation along the shorter arc, the sample count raised by the arc a sphere at the table's reach
// travels), evaluated as the body call evaluates a pose, and reduced in registers; per path a few words leave the device.
//   k_path_check     (path_kernels.hpp; device variant only) offsets against the CSR rules, per path
//   k_sweep_plan     one wave per path: a lane per waypoint normalises its quaternion (stored: `uq`) and computes its segment's S; the
//                    int64 wave scan gives every waypoint's first sample index (`base`), the path's n_samples and its validity
//   k_sweep_pieces   one work-group: piece counts scanned over the paths; the total stays on the device
//   k_sweep_eval     persistent grid of 256-thread work-groups, one wave per piece.  The sphere table lies once per work-group in LDS,
//                    one array per component (k_body_eval's layout).  A TEAM of T lanes per sample (body_team_shift), 64 / T
//                    consecutive samples per wave and trip; the sample -> segment lookup is k_path_eval's: one coalesced load of 64
//                    first-sample indices and a 6-step search through __shfl, no dependent global loads.  Every lane of a team builds
//                    the sample's pose and rotation, lane t takes spheres t, t + T, ...; the xor butterfly over the team gives the
//                    sample's minimum (s, sphere) and its lowest sphere below the margin; the team keeps, in sample order, a running
//                    minimum (s, sample, sphere), the first sample below (sample, sphere) and the count of samples below; a butterfly
//                    over the wave's teams (value, then sample index) leaves one record per piece
//   k_sweep_finish   one lane per path: its piece records in index order, then the winner's pose, position and gradient and the
//                    first-below pose, each recomputed once by the rule
// No atomics at all: the result depends neither on the launch shape, nor on the piece size, nor on scheduling.  The call -- result
// struct, scalars, scratch pointers -- and the table reach the map's scratch in one stream-ordered copy and are read where they are
// used: every kernel takes one pointer (body_kernels.hpp records what the alternative spilled).
#pragma once
#include <cstring>
#include <vector>

#include "body_kernels.hpp"
#include "path_kernels.hpp"

namespace fiesta {
namespace {  // (planner.hip alone includes this header; the namespace is part of the kernels' symbol names)

constexpr int kSweepTrips = 16;  // trips of a wave per piece at least: a piece holds kSweepTrips * 64 / T samples or more

struct SweepRec {  // one piece: its minimum with sample and sphere, the first sample below the margin with its lowest such sphere
  double v;        // (LLONG_MAX: none), the samples below
  long long i, fb, nb;
  int sph, fbs;
};

struct SweepCall {  // the call as the kernels read it, at the start of the map's scratch; the table follows it
  fiesta_hip_sweep_result r;
  const double *poses;  // n_poses x 7
  const int64_t *off;   // n_paths + 1, as the caller gave them
  const double *sph;    // the table: cx, cy, cz, r per sphere
  double *uq;           // n_poses x 4: the waypoints' normalised quaternions
  int64_t *base, *nsamp, *rng, *poff;
  SweepRec *rec;
  int64_t n_poses, n_paths;
  long long max_pieces, min_piece;
  double step, margin, reach225;  // reach225 = 2.25 * reach
  int K, shift, checked, pad;
};

// ---- the rule (include/fiesta_hip.h) -----------------------------------------------------------------------------------------------
// a waypoint pose's validity (the body call's) and its normalised quaternion
__device__ inline bool sweep_unit(const double *pose, double *u) {
  const double qw = pose[3], qx = pose[4], qy = pose[5], qz = pose[6];
  const double s = ((qw * qw + qx * qx) + qy * qy) + qz * qz;
  const double k = 2.0 / s;
  bool valid = s > 0 && __builtin_isfinite(k);
#pragma unroll
  for (int c = 0; c < 7; ++c) valid = valid && __builtin_isfinite(pose[c]);
  const double n = sqrt(s);
  u[0] = qw / n, u[1] = qx / n, u[2] = qy / n, u[3] = qz / n;
  return valid;
}
// segment (a, u0) -> (b, u1): d = b - a and v, u1 on u0's side
__device__ inline void sweep_arc(const double *a, const double *u0, const double *b, const double *u1, double *d, double *v) {
#pragma unroll
  for (int c = 0; c < 3; ++c) d[c] = b[c] - a[c];
  const double dot = ((u0[0] * u1[0] + u0[1] * u1[1]) + u0[2] * u1[2]) + u0[3] * u1[3];
  const bool same = dot >= 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) v[c] = same ? u1[c] : -u1[c];
}
// its S; false if (L + W) / step > 2^24 (or is not a number)
__device__ inline bool sweep_segment_samples(const double *d, const double *u0, const double *v, double reach225, double step, long long *S) {
  const double L = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  const double e0 = v[0] - u0[0], e1 = v[1] - u0[1], e2 = v[2] - u0[2], e3 = v[3] - u0[3];
  const double ch = sqrt(((e0 * e0 + e1 * e1) + e2 * e2) + e3 * e3);
  const double W = reach225 * ch;
  const double q = (L + W) / step;
  if (!(q <= kPathMaxRatio)) return false;
  const long long s = (long long)ceil(q);
  *S = s < 1 ? 1 : s;
  return true;
}
// sample k of S of the segment
__device__ inline void sweep_pose(const double *a, const double *u0, const double *d, const double *v, long long k, long long S, double *pose) {
  const double t = (double)k / (double)S;
  const double r = 1.0 - t;
#pragma unroll
  for (int c = 0; c < 3; ++c) pose[c] = a[c] + d[c] * t;
#pragma unroll
  for (int c = 0; c < 4; ++c) pose[3 + c] = r * u0[c] + t * v[c];
}
// sample k of S of the segment that starts at waypoint j of a path of nw poses w with normalised quaternions u
__device__ inline void sweep_sample(const double *w, const double *u, int64_t nw, int64_t j, long long k, long long S, double *pose) {
  const double *a = w + 7 * j, *u0 = u + 4 * j;
  if (j == nw - 1) {  // the final sample: the last waypoint's position with its own u
    pose[0] = a[0], pose[1] = a[1], pose[2] = a[2], pose[3] = u0[0], pose[4] = u0[1], pose[5] = u0[2], pose[6] = u0[3];
    return;
  }
  double d[3], v[4];
  sweep_arc(a, u0, a + 7, u0 + 4, d, v);
  sweep_pose(a, u0, d, v, k, S, pose);
}
// the body call's rotation of a pose
__device__ inline void sweep_rotation(const double *pose, double R[3][3]) {
  const double qw = pose[3], qx = pose[4], qy = pose[5], qz = pose[6];
  const double s = ((qw * qw + qx * qx) + qy * qy) + qz * qz;
  const double k = 2.0 / s;
  const double xx = qx * qx, yy = qy * qy, zz = qz * qz, xy = qx * qy, xz = qx * qz, yz = qy * qz, wx = qw * qx, wy = qw * qy, wz = qw * qz;
  R[0][0] = 1.0 - k * (yy + zz), R[0][1] = k * (xy - wz), R[0][2] = k * (xz + wy);
  R[1][0] = k * (xy + wz), R[1][1] = 1.0 - k * (xx + zz), R[1][2] = k * (yz - wx);
  R[2][0] = k * (xz - wy), R[2][1] = k * (yz + wx), R[2][2] = 1.0 - k * (xx + yy);
}
// samples per piece of a path of n samples: at least min_piece, and at most max_pieces pieces
__device__ inline long long sweep_piece_size(long long n, long long max_pieces, long long min_piece) {
  const long long ps = (n + max_pieces - 1) / max_pieces;
  return ps < min_piece ? min_piece : ps;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------------
// one wave per path: uq[i] = waypoint i's normalised quaternion, base[i] = index of its first sample in its path, nsamp[p] = n_samples
// (-1: invalid, 0: empty).  Host variant (offsets checked on the host): rng is written here.
__global__ __launch_bounds__(256) void k_sweep_plan(const SweepCall *cp) {
  const int64_t p = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  const int checked = cp->checked;
  int64_t *const nsamp = cp->nsamp, *const rng = cp->rng;
  if (p >= cp->n_paths) return;         // (uniform in the wave)
  if (checked && nsamp[p] < 0) return;  // offsets out of order or out of range (k_path_check)
  const int64_t o0 = checked ? rng[2 * p] : cp->off[p], o1 = checked ? rng[2 * p + 1] : cp->off[p + 1];
  if (!checked && lane == 0) rng[2 * p] = o0, rng[2 * p + 1] = o1;
  const double *const poses = cp->poses;
  const double step = cp->step, reach225 = cp->reach225;
  long long carry = 0;
  int bad = 0;
  for (int64_t c = o0; c < o1; c += 64) {
    const int64_t i = c + lane;
    long long S = 0;
    int lane_bad = 0;
    if (i < o1) {
      const double *a = poses + 7 * i;
      double u0[4];
      lane_bad = !sweep_unit(a, u0);
#pragma unroll
      for (int k = 0; k < 4; ++k) cp->uq[4 * i + k] = u0[k];
      if (i + 1 < o1) {
        double u1[4], d[3], v[4];
        if (!sweep_unit(a + 7, u1)) lane_bad = 1;  // (the same bits the next lane stores)
        sweep_arc(a, u0, a + 7, u1, d, v);
        if (!sweep_segment_samples(d, u0, v, reach225, step, &S)) lane_bad = 1;
      }
    }
    const long long incl = wave_inclusive_sum(S);
    if (i < o1) cp->base[i] = carry + incl - S;
    carry += __shfl(incl, 63, 64);
    bad |= __any(lane_bad);
  }
  if (lane == 0) nsamp[p] = bad ? -1 : (o1 > o0 ? carry + 1 : 0);
}

// one work-group: poff[p] = first piece of path p, poff[n_paths] = pieces in total (read by k_sweep_eval, never by the host)
__global__ __launch_bounds__(1024) void k_sweep_pieces(const SweepCall *cp) {
  __shared__ long long lds[16];
  const int64_t *const nsamp = cp->nsamp;
  int64_t *const poff = cp->poff;
  const int64_t n_paths = cp->n_paths;
  const long long max_pieces = cp->max_pieces, min_piece = cp->min_piece;
  const long long total = block_scan_stride<1, 16>(
      n_paths, lds,
      [&](int64_t p) {
        const long long n = nsamp[p];
        if (n <= 0) return 0ll;
        const long long ps = sweep_piece_size(n, max_pieces, min_piece);
        return (n + ps - 1) / ps;
      },
      [&](int64_t p, long long first, long long) { poff[p] = first; });
  if (threadIdx.x == 0) poff[n_paths] = total;
}

// Dynamic LDS: 4 * K doubles
template <class Eval>
__global__ __launch_bounds__(256) void k_sweep_eval(Eval ev, const SweepCall *cp) {
  extern __shared__ double sweep_tab[];  // cx[K], cy[K], cz[K], r[K]
  const int K = cp->K, shift = cp->shift;
  {
    const double *const sph = cp->sph;
    for (int i = threadIdx.x; i < 4 * K; i += 256) sweep_tab[(i & 3) * K + (i >> 2)] = sph[i];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, T = 1 << shift, t = lane & (T - 1), per = 64 >> shift, team = lane >> shift;
  const int64_t n_paths = cp->n_paths;
  const int64_t *const poff = cp->poff;
  const int64_t total = poff[n_paths];
  const int64_t stride = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t piece = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6; piece < total; piece += stride) {  // (uniform in the wave)
    const int64_t p = path_find(poff, 0, n_paths - 1, piece);  // the last path that starts at or before this piece (it has pieces)
    const long long n = cp->nsamp[p], ps = sweep_piece_size(n, cp->max_pieces, cp->min_piece);
    const long long s0 = (piece - poff[p]) * ps, s1 = s0 + ps < n ? s0 + ps : n;
    const int64_t o0 = cp->rng[2 * p], nw = cp->rng[2 * p + 1] - o0;
    const double *const pw = cp->poses + 7 * o0, *const pu = cp->uq + 4 * o0;
    const int64_t *const pb = cp->base + o0;
    const double margin = cp->margin;
    int64_t jw = path_find(pb, 0, nw - 1, s0);  // the segment of the trip's first sample (uniform in the wave)
    double best = INFINITY;
    long long bs = LLONG_MAX, fb = LLONG_MAX, nb = 0;
    int bsph = -1, fbs = -1;
    for (long long sg = s0; sg < s1; sg += per) {  // (every lane takes part in the shuffles, also past s1)
      const long long s = sg + team;
      const long long bl = jw + lane < nw ? pb[jw + lane] : LLONG_MAX;  // first samples of segments jw .. jw + 63
      const long long bn = jw + 64 < nw ? pb[jw + 64] : LLONG_MAX;
      int i = 0;  // the last i with b_i <= s (b_0 <= sg <= s): exactly 6 halvings of [0, 63]
      for (int h = 32; h > 0; h >>= 1) {
        const long long bm = __shfl(bl, i + h, 64);
        if (bm <= s) i += h;
      }
      const long long bj = __shfl(bl, i, 64), nx = __shfl(bl, i < 63 ? i + 1 : 63, 64);
      const long long end = i < 63 ? nx : bn;  // first sample of segment j + 1
      const int64_t j = jw + i;
      const bool have = s < s1;
      double pose[7] = {0, 0, 0, 1, 0, 0, 0}, R[3][3];
      if (have) sweep_sample(pw, pu, nw, j, s - bj, end - bj, pose);
      sweep_rotation(pose, R);
      double bv = INFINITY;  // this lane's minimum over its spheres: (value, sphere), smaller value, then smaller sphere
      int bi = INT_MAX, fs = INT_MAX;  // fs: its lowest sphere below the margin
      for (int i0 = 0; i0 < K; i0 += T) {  // (uniform: a lane past the table or past s1 contributes the identity)
        const int k = i0 + t;
        if (have && k < K) {
          const double cx = sweep_tab[k], cy = sweep_tab[K + k], cz = sweep_tab[2 * K + k], rad = sweep_tab[3 * K + k];
          double x[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) x[c] = pose[c] + ((R[c][0] * cx + R[c][1] * cy) + R[c][2] * cz);
          const double si = ev(x, nullptr) - rad;
          if (bi == INT_MAX || si < bv) bv = si, bi = k;  // (this lane's spheres only grow; its first one always counts)
          if (fs == INT_MAX && si < margin) fs = k;
        }
      }
      for (int o = T >> 1; o > 0; o >>= 1) {  // wave_reduce's butterfly, limited to the team
        const double ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64), of = __shfl_xor(fs, o, 64);
        if (oi != INT_MAX && (bi == INT_MAX || ov < bv || (ov == bv && oi < bi))) bv = ov, bi = oi;
        fs = of < fs ? of : fs;
      }
      if (have) {  // (the team's samples grow: a tie keeps the lower one)
        if (bs == LLONG_MAX || bv < best) best = bv, bs = s, bsph = bi;
        if (fs != INT_MAX) {
          if (fb == LLONG_MAX) fb = s, fbs = fs;
          ++nb;
        }
      }
      // the next trip's first sample sg + per lies in lane 63's segment, or in the one after it if that segment ends at sg + per - 1:
      // its window must start exactly there
      jw = (int64_t)__shfl((long long)j, 63, 64) + (sg + per >= __shfl(end, 63, 64) ? 1 : 0);
    }
    for (int o = 32; o >= T; o >>= 1) {  // over the wave's teams (every lane of a team holds the team's values)
      const double ov = __shfl_xor(best, o, 64);
      const long long oi = __shfl_xor(bs, o, 64), of = __shfl_xor(fb, o, 64), on = __shfl_xor(nb, o, 64);
      const int osph = __shfl_xor(bsph, o, 64), ofs = __shfl_xor(fbs, o, 64);
      if (oi != LLONG_MAX && (bs == LLONG_MAX || ov < best || (ov == best && oi < bs))) best = ov, bs = oi, bsph = osph;
      if (of < fb) fb = of, fbs = ofs;
      nb += on;
    }
    if (lane == 0) cp->rec[piece] = SweepRec{best, bs, fb, nb, bsph, fbs};
  }
}

template <class Eval>
__global__ __launch_bounds__(256) void k_sweep_finish(Eval ev, const SweepCall *cp) {
  const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (p >= cp->n_paths) return;
  const long long n = cp->nsamp[p];
  const double nan = NAN;
  double md = n < 0 ? nan : (double)INFINITY;
  long long mi = -1, fi = -1, nb = n < 0 ? -1 : 0;
  int ms = -1, fs = -1;
  double mpose[7], fpose[7], mp[3] = {nan, nan, nan}, g[3] = {0, 0, 0};
#pragma unroll
  for (int c = 0; c < 7; ++c) mpose[c] = fpose[c] = nan;
  if (n > 0) {
    const int64_t *const poff = cp->poff;
    const SweepRec *const rec = cp->rec;
    for (int64_t k = poff[p]; k < poff[p + 1]; ++k) {  // in index order: a strictly smaller value wins, a tie keeps the earlier piece
      const SweepRec e = rec[k];
      if (mi < 0 || e.v < md) md = e.v, mi = e.i, ms = e.sph;
      if (fi < 0 && e.fb != LLONG_MAX) fi = e.fb, fs = e.fbs;
      nb += e.nb;
    }
    const int64_t o0 = cp->rng[2 * p], nw = cp->rng[2 * p + 1] - o0;
    const double *const pw = cp->poses + 7 * o0, *const pu = cp->uq + 4 * o0;
    const int64_t *const pb = cp->base + o0;
    int64_t j = path_find(pb, 0, nw - 1, mi);
    sweep_sample(pw, pu, nw, j, mi - pb[j], j + 1 < nw ? pb[j + 1] - pb[j] : 1, mpose);
    double R[3][3];
    sweep_rotation(mpose, R);
    const double *const c = cp->sph + 4 * ms;
#pragma unroll
    for (int k = 0; k < 3; ++k) mp[k] = mpose[k] + ((R[k][0] * c[0] + R[k][1] * c[1]) + R[k][2] * c[2]);
    (void)ev(mp, g);  // the gradient of the point query at the winning sphere (its value less the radius is the minimum, bit for bit)
    if (fi >= 0) {
      j = path_find(pb, 0, nw - 1, fi);
      sweep_sample(pw, pu, nw, j, fi - pb[j], j + 1 < nw ? pb[j + 1] - pb[j] : 1, fpose);
    }
  }
  const fiesta_hip_sweep_result r = cp->r;
  if (r.min_clearance) r.min_clearance[p] = md;
  if (r.min_sample) r.min_sample[p] = mi;
  if (r.min_sphere) r.min_sphere[p] = ms;
  if (r.first_below) r.first_below[p] = fi;
  if (r.first_below_sphere) r.first_below_sphere[p] = fs;
  if (r.n_below) r.n_below[p] = nb;
  if (r.n_samples) r.n_samples[p] = n;
#pragma unroll
  for (int c = 0; c < 7; ++c) {
    if (r.min_pose) r.min_pose[7 * p + c] = mpose[c];
    if (r.first_below_pose) r.first_below_pose[7 * p + c] = fpose[c];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (r.min_pos) r.min_pos[3 * p + c] = mp[c];
    if (r.min_grad) r.min_grad[3 * p + c] = g[c];
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
// the table's reach: the farthest sphere centre from the body origin (fiesta_amd.body_reach)
inline double sweep_reach(const double *sph, int K) {
  double reach = 0;
  for (int i = 0; i < K; ++i) {
    const double cx = sph[4 * i], cy = sph[4 * i + 1], cz = sph[4 * i + 2];
    reach = std::max(reach, std::sqrt((cx * cx + cy * cy) + cz * cz));
  }
  return reach;
}

// The device pipeline.  poses / off / r are device pointers (the host variant has staged them); tmp is the map's grow-only scratch:
// the call and the table, the plan, the piece records.  Every grid size follows from n_paths alone: nothing is read back.  One copy
// on the stream from a block of pageable host memory: it has left the host when the copy call returns.
template <class Eval>
void sweep_launch(hipStream_t st, DevBuf<unsigned char> &tmp, const Eval &ev, const SweepArgs &a, const double *poses, const int64_t *off,
                  bool checked, const fiesta_hip_sweep_result &r) {
  const int K = a.n_spheres, shift = body_team_shift(K);
  const long long max_pieces = std::max<int64_t>(1, kPathRecords / a.n_paths);
  const int64_t nrec = a.n_paths * max_pieces;  // <= max(kPathRecords, n_paths)
  const size_t np = (size_t)a.n_poses, n = (size_t)a.n_paths, tab = (size_t)K * 4 * sizeof(double);
  const size_t b_sph = sizeof(SweepCall), b_uq = b_sph + tab, b_base = b_uq + np * 32, b_nsamp = b_base + np * 8, b_rng = b_nsamp + n * 8,
               b_poff = b_rng + n * 16, b_rec = b_poff + (n + 1) * 8, bytes = b_rec + (size_t)nrec * sizeof(SweepRec);
  static_assert(sizeof(SweepCall) % 8 == 0 && sizeof(SweepRec) % 8 == 0, "the scratch sections are 8-byte aligned");
  tmp.ensure(bytes, st);
  SweepCall c{};
  c.r = r, c.poses = poses, c.off = off, c.sph = (const double *)(tmp.p + b_sph), c.uq = (double *)(tmp.p + b_uq);
  c.base = (int64_t *)(tmp.p + b_base), c.nsamp = (int64_t *)(tmp.p + b_nsamp), c.rng = (int64_t *)(tmp.p + b_rng);
  c.poff = (int64_t *)(tmp.p + b_poff), c.rec = (SweepRec *)(tmp.p + b_rec);
  c.n_poses = a.n_poses, c.n_paths = a.n_paths, c.max_pieces = max_pieces, c.min_piece = (long long)kSweepTrips * (64 >> shift);
  c.step = a.step, c.margin = a.margin, c.reach225 = 2.25 * sweep_reach(a.spheres, K);
  c.K = K, c.shift = shift, c.checked = checked ? 1 : 0;
  std::vector<unsigned char> head(b_uq);
  memcpy(head.data(), &c, sizeof(c)), memcpy(head.data() + b_sph, a.spheres, tab);
  FIESTA_HIP_CHECK(hipMemcpyAsync(tmp.p, head.data(), head.size(), hipMemcpyHostToDevice, st));
  const SweepCall *cp = (const SweepCall *)tmp.p;
  if (checked) hipLaunchKernelGGL(k_path_check, dim3(1), dim3(1024), 0, st, off, a.n_paths, a.n_poses, c.nsamp, c.rng);
  hipLaunchKernelGGL(k_sweep_plan, dim3((unsigned)((a.n_paths + 3) / 4)), dim3(256), 0, st, cp);
  hipLaunchKernelGGL(k_sweep_pieces, dim3(1), dim3(1024), 0, st, cp);
  hipLaunchKernelGGL(k_sweep_eval<Eval>, dim3(kBodyBlocks), dim3(256), tab, st, ev, cp);
  hipLaunchKernelGGL(k_sweep_finish<Eval>, dim3((unsigned)((a.n_paths + 255) / 256)), dim3(256), 0, st, ev, cp);
  FIESTA_HIP_CHECK(hipGetLastError());
}

// Both variants of the call on a map's stream.  The device variant only enqueues; the host variant stages the poses and offsets
// through S.in and every output through S.out, synchronises and copies back.  It always runs on the device.
template <class Eval>
void body_sweep_run(hipStream_t st, PlannerScratch &S, const Eval &ev, const SweepArgs &a) {
  const fiesta_hip_sweep_result &r = *a.res;
  if (a.dev) return sweep_launch(st, S.tmp, ev, a, a.poses, a.off, true, r);
  const size_t n = (size_t)a.n_paths, np7 = (size_t)a.n_poses * 7;
  Staging in{S.in, st}, out{S.out, st};
  const auto poses = in.add(a.poses, np7);
  const auto off = in.add(a.off, n + 1);
  in.alloc(), in.up(poses, np7), in.up(off, n + 1);
  const auto min_clearance = out.add(r.min_clearance, n);
  const auto min_sample = out.add(r.min_sample, n);
  const auto min_sphere = out.add(r.min_sphere, n);
  const auto min_pose = out.add(r.min_pose, 7 * n), min_pos = out.add(r.min_pos, 3 * n), min_grad = out.add(r.min_grad, 3 * n);
  const auto first_below = out.add(r.first_below, n);
  const auto first_below_sphere = out.add(r.first_below_sphere, n);
  const auto first_below_pose = out.add(r.first_below_pose, 7 * n);
  const auto n_below = out.add(r.n_below, n), n_samples = out.add(r.n_samples, n);
  out.alloc();
  const fiesta_hip_sweep_result d{out.dev(min_clearance), out.dev(min_sample),        out.dev(min_sphere),       out.dev(min_pose),
                                  out.dev(min_pos),       out.dev(min_grad),          out.dev(first_below),      out.dev(first_below_sphere),
                                  out.dev(first_below_pose), out.dev(n_below),        out.dev(n_samples)};
  sweep_launch(st, S.tmp, ev, a, in.dev(poses), in.dev(off), false, d);
  out.back(min_clearance, n), out.back(min_sample, n), out.back(min_sphere, n), out.back(min_pose, 7 * n), out.back(min_pos, 3 * n);
  out.back(min_grad, 3 * n), out.back(first_below, n), out.back(first_below_sphere, n), out.back(first_below_pose, 7 * n);
  out.back(n_below, n), out.back(n_samples, n);
  FIESTA_HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace
}  // namespace fiesta
