// fiesta_amd/csrc/articulated_kernels.hpp -- articulated body queries: spheres on frames, one pose per frame and configuration:
// fiesta_hip_articulated_query / _dev (include/fiesta_hip.h).
//
// The body call (body_kernels.hpp) moves one rigid set of spheres.  An arm, a drone with a slung load or a formation is several rigid
// sets -- links, FRAMES -- and a planner that checks it link by link pays one call per link and reduces across the links itself.  Here
// every sphere of the table names its frame, a CONFIGURATION gives one pose per frame, and one launch returns the configuration's
// minimum, count and cost and, per frame, the clearance, the cost and the force and torque on that frame.  A sphere's arithmetic is
// the body call's, operation by operation, with R and p of the sphere's frame.
//   k_artic_eval  persistent grid, a TEAM of T lanes per configuration (T as in k_body_eval).  The sphere table and its frame
//                 indices lie once per work-group in LDS.  Per trip a team builds its configuration's F transforms (R, p: 12 doubles)
//                 into LDS, lane t the frames t, t + T, ...: the rotation and its division are paid once per frame, and validity is
//                 the AND over the frames, a butterfly over the team.  The evaluation loop is the body call's: lane t takes spheres
//                 t, t + T, ... at full lane use whatever the frame sizes are.  The table is grouped by frame and shared by every
//                 team, so the frames that a pass of T spheres spans are uniform in the work-group: per frame of the span one masked
//                 xor butterfly over the team (lanes of other frames contribute +0 / +inf) adds into a running accumulator of seven
//                 sums and a minimum, which is stored when the span has moved past the frame.  cost is the frame costs added in
//                 frame order.  The minimum over all spheres is kept as in k_body_eval.
// No floating-point atomics, no scratch buffer, no second kernel.  The order of every sum follows from n_spheres and sphere_frame
// alone: the bits of a configuration's outputs depend neither on n_configs, nor on its place in the batch, nor on the grid.
#pragma once
#include <cstring>
#include <vector>

#include "body_kernels.hpp"

namespace fiesta {
namespace {  // (planner.hip alone includes this header; the namespace is part of the kernels' symbol names)

constexpr int kArticBlocks = 1024;         // persistent grid of k_artic_eval, as k_body_eval's
constexpr size_t kArticLds = 64 * 1024;    // table + transforms stay within the default dynamic LDS limit: two work-groups per CU and more

// the bytes of the sphere table in LDS: four doubles and the frame index per sphere, the transforms behind it 8-byte aligned
inline size_t artic_table_bytes(int K) { return (size_t)K * 32 + (size_t)((K + 1) & ~1) * 4; }
// configurations per work-group and trip: a team each, capped so that their transforms (96 B per frame) fit beside the table
inline int artic_per_trip(int K, int F) {
  const size_t cap = (kArticLds - artic_table_bytes(K)) / ((size_t)F * 96);
  return (int)std::min<size_t>(256 >> body_team_shift(K), cap);
}

// What the kernel reads of a call besides the table, on the device behind it: read where it is used.  (k_body_eval's finding: as
// kernel arguments the result pointers stay in scalar registers across the sphere loop, next to the evaluator's geometry, and spill;
// here the poses, the count and the margin do so as well.)
struct ArticCall {
  fiesta_hip_articulated_result r;
  const double *poses;
  int64_t n_configs, groups;  // groups: the trips of the whole grid, ceil(n_configs / per)
  int32_t grid;               // its work-groups
  double margin;
};

// sph, frm: the table as the caller gave it, on the device.  Dynamic LDS: cx[K], cy[K], cz[K], r[K], frame[K] (padded to an even
// count), then per * F transforms of 12 doubles (R row-major, p).
template <class Eval>
__global__ __launch_bounds__(256) void k_artic_eval(Eval ev, const double *sph, const int32_t *frm, int K, int F, int shift, int per,
                                                    const ArticCall *call) {
  extern __shared__ double artic_lds[];
  double *const tab = artic_lds;                                 // cx[K], cy[K], cz[K], r[K]
  int32_t *const frame = (int32_t *)(artic_lds + 4 * (size_t)K);  // frame[K]
  double *const tf_all = artic_lds + 4 * (size_t)K + ((K + 1) >> 1);
  for (int i = threadIdx.x; i < 4 * K; i += 256) tab[(i & 3) * K + (i >> 2)] = sph[i];
  for (int i = threadIdx.x; i < K; i += 256) frame[i] = frm[i];
  const int T = 1 << shift;
  for (int64_t grp = blockIdx.x; grp < call->groups; grp += (uint32_t)__builtin_amdgcn_readfirstlane(call->grid)) {  // (uniform in the work-group)
    __syncthreads();  // the table is there; the trip before has read its transforms
    // The lane id is taken anew in every trip, through an empty asm the compiler cannot look behind: what derives from it (the
    // lane's masks, the strides of p * F and p * K from trip to trip) would otherwise be kept across the trips in scalar registers,
    // next to the evaluator's geometry, and the dense kernel spilled 16 of them.  It costs a few integer operations per trip.
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int t = tid & (T - 1), slot = tid >> shift;
    double *const tf = tf_all + (size_t)(slot < per ? slot : 0) * F * 12;  // this team's transforms (teams past the cap idle)
    const int64_t p = grp * (uint32_t)per + slot;  // (unsigned factors: no sign words to keep)
    const bool have = slot < per && p < call->n_configs;
    int ok = have;
    if (have) {
      const double *const poses = call->poses + p * (uint32_t)F * 7;
      for (int f = t; f < F; f += T) {
        double q[7];
#pragma unroll
        for (int c = 0; c < 7; ++c) q[c] = poses[f * 7 + c];
        const double qw = q[3], qx = q[4], qy = q[5], qz = q[6];
        const double s = ((qw * qw + qx * qx) + qy * qy) + qz * qz;
        const double k = 2.0 / s;
        bool valid = s > 0 && __builtin_isfinite(k);
#pragma unroll
        for (int c = 0; c < 7; ++c) valid = valid && __builtin_isfinite(q[c]);
        ok &= (int)valid;
        const double xx = qx * qx, yy = qy * qy, zz = qz * qz, xy = qx * qy, xz = qx * qz, yz = qy * qz, wx = qw * qx, wy = qw * qy, wz = qw * qz;
        double *const o = tf + 12 * f;
        o[0] = 1.0 - k * (yy + zz), o[1] = k * (xy - wz), o[2] = k * (xz + wy);
        o[3] = k * (xy + wz), o[4] = 1.0 - k * (xx + zz), o[5] = k * (yz - wx);
        o[6] = k * (xz - wy), o[7] = k * (yz + wx), o[8] = 1.0 - k * (xx + yy);
        o[9] = q[0], o[10] = q[1], o[11] = q[2];
      }
    }
    for (int o = T >> 1; o > 0; o >>= 1) ok &= __shfl_xor(ok, o, 64);  // a configuration is valid iff all its frames are
    const bool valid = ok != 0;
    __syncthreads();  // the transforms are there
    double bv = INFINITY, bx[3] = {NAN, NAN, NAN}, bg[3] = {NAN, NAN, NAN};  // this lane's minimum, as in k_body_eval
    int bi = INT_MAX, nb = 0;
    double run[7] = {0, 0, 0, 0, 0, 0, 0}, run_min = INFINITY, cost = 0;  // the frame `cur` so far; the frame costs so far
    int cur = 0;                                                           // the frames below cur are stored
    // frame f is complete: the team's first lane stores its three rows and adds its cost
    auto emit = [&](int f) {
      cost = cost + run[0];
      if (have && t == 0) {
        double *const fclear = call->r.frame_clearance, *const fcost = call->r.frame_cost, *const fgrad = call->r.frame_grad;
        const int64_t row = p * (uint32_t)F + f;
        if (fclear) fclear[row] = valid ? run_min : NAN;
        if (fcost) fcost[row] = valid ? run[0] : NAN;
        if (fgrad) {
#pragma unroll
          for (int c = 0; c < 6; ++c) fgrad[6 * row + c] = valid ? run[1 + c] : 0.0;
        }
      }
#pragma unroll
      for (int c = 0; c < 7; ++c) run[c] = 0;
      run_min = INFINITY;
    };
    double *clearance = call->r.sphere_clearance;
    if (clearance) clearance += p * (uint32_t)K;
    int i0 = 0;
    do {  // (uniform: a lane past the table or of an invalid configuration contributes the identity; K >= 1)
      const int i = i0 + t;
      const bool mine = valid && i < K;
      const int myf = i < K ? frame[i] : -1;
      double term[7] = {0, 0, 0, 0, 0, 0, 0}, si = INFINITY;
      if (mine) {
        const double cx = tab[i], cy = tab[K + i], cz = tab[2 * K + i], rad = tab[3 * K + i];
        const double *const R = tf + 12 * myf;
        double a[3], x[3], g[3], phi, gam[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          a[c] = (R[3 * c] * cx + R[3 * c + 1] * cy) + R[3 * c + 2] * cz;
          x[c] = R[9 + c] + a[c];
        }
        const double d = ev(x, g);
        si = d - rad;
        nb += cost_penalty(si, g, call->margin, &phi, gam);
        term[0] = phi;
        term[1] = gam[0], term[2] = gam[1], term[3] = gam[2];
        term[4] = a[1] * gam[2] - a[2] * gam[1];
        term[5] = a[2] * gam[0] - a[0] * gam[2];
        term[6] = a[0] * gam[1] - a[1] * gam[0];
        if (si < bv) {  // (this lane's indices only grow)
          bv = si, bi = i;
#pragma unroll
          for (int c = 0; c < 3; ++c) bx[c] = x[c], bg[c] = g[c];
        }
        if (clearance) clearance[i] = si;
      } else if (have && i < K && clearance) {
        clearance[i] = NAN;  // (an invalid configuration's row)
      }
      // the frames of this pass: f_lo .. f_hi, of which f_hi goes on in the next pass iff that one starts with it (all uniform in
      // the work-group: the table is shared)
      const int last = (i0 + T < K ? i0 + T : K) - 1;
      const int f_lo = __builtin_amdgcn_readfirstlane(frame[i0]), f_hi = __builtin_amdgcn_readfirstlane(frame[last]);
      const int nxt = __builtin_amdgcn_readfirstlane(i0 + T < K ? frame[i0 + T] : F);
      for (int f = cur; f <= f_hi; ++f) {
        if (f >= f_lo) {  // (a frame below f_lo has no sphere here: it is empty, or complete since the pass before)
          const bool in = mine && myf == f;
          double v[7], mn = in ? si : INFINITY;
#pragma unroll
          for (int c = 0; c < 7; ++c) v[c] = in ? term[c] : 0.0;
          for (int o = T >> 1; o > 0; o >>= 1) {  // wave_reduce's butterfly, limited to the team
#pragma unroll
            for (int c = 0; c < 7; ++c) v[c] = v[c] + __shfl_xor(v[c], o, 64);
            const double om = __shfl_xor(mn, o, 64);
            mn = om < mn ? om : mn;
          }
#pragma unroll
          for (int c = 0; c < 7; ++c) run[c] = run[c] + v[c];
          run_min = mn < run_min ? mn : run_min;
        }
        if (f < nxt) emit(f);
      }
      cur = nxt == f_hi ? f_hi : f_hi + 1;
      i0 += T;
    } while (i0 < K);
    for (int f = cur; f < F; ++f) emit(f);  // the frames behind the last sphere's own no sphere
    for (int o = T >> 1; o > 0; o >>= 1) {
      nb += __shfl_xor(nb, o, 64);
      const double ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov < bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
    }
    if (have) {
      const fiesta_hip_articulated_result r = call->r;
      if (valid) {
        if (t == 0) {
          if (r.min_clearance) r.min_clearance[p] = bv;
          if (r.min_sphere) r.min_sphere[p] = bi;
          if (r.n_below) r.n_below[p] = nb;
          if (r.cost) r.cost[p] = cost;
        }
        if (t == (bi & (T - 1))) {  // sphere bi is this lane's, and this lane's minimum is the team's
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            if (r.min_pos) r.min_pos[3 * p + c] = bx[c];
            if (r.min_grad) r.min_grad[3 * p + c] = bg[c];
          }
        }
      } else {
        if (t == 0) {
          if (r.min_clearance) r.min_clearance[p] = NAN;
          if (r.min_sphere) r.min_sphere[p] = -1;
          if (r.n_below) r.n_below[p] = -1;
          if (r.cost) r.cost[p] = NAN;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            if (r.min_pos) r.min_pos[3 * p + c] = NAN;
            if (r.min_grad) r.min_grad[3 * p + c] = NAN;
          }
        }
      }
    }
  }
}

// The call's header in the map's scratch -- the sphere table, the frame indices (padded to an even count), then the ArticCall with
// the result struct `r` of device pointers -- and the launch.  One copy on the stream from a block of pageable host memory: it has
// left the host when the copy call returns.
template <class Eval>
void artic_enqueue(hipStream_t st, DevBuf<unsigned char> &tmp, const Eval &ev, const ArticulatedArgs &a, const double *poses,
                   const fiesta_hip_articulated_result &r) {
  const int K = a.n_spheres, F = a.n_frames, shift = body_team_shift(K), per = artic_per_trip(K, F);
  const size_t tab = (size_t)K * 4 * sizeof(double), frames = (size_t)((K + 1) & ~1) * sizeof(int32_t);
  const size_t lds = artic_table_bytes(K) + (size_t)per * F * 96;
  const unsigned grid = (unsigned)std::min<int64_t>((a.n_configs + per - 1) / per, kArticBlocks);
  const ArticCall call{r, poses, a.n_configs, (a.n_configs + per - 1) / per, (int32_t)grid, a.margin};
  std::vector<unsigned char> head(tab + frames + sizeof(call));
  memcpy(head.data(), a.spheres, tab), memcpy(head.data() + tab, a.sphere_frame, (size_t)K * sizeof(int32_t));
  memcpy(head.data() + tab + frames, &call, sizeof(call));
  tmp.ensure(head.size(), st);
  FIESTA_HIP_CHECK(hipMemcpyAsync(tmp.p, head.data(), head.size(), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_artic_eval<Eval>, dim3(grid), dim3(256), lds, st, ev, (const double *)tmp.p, (const int32_t *)(tmp.p + tab), K, F, shift,
                     per, (const ArticCall *)(tmp.p + tab + frames));
  FIESTA_HIP_CHECK(hipGetLastError());
}

// Both variants of the call on a map's stream.  The device variant only enqueues; the host variant stages the frame poses through
// S.in and every output through S.out, synchronises and copies back.  It always runs on the device.
template <class Eval>
void articulated_query_run(hipStream_t st, PlannerScratch &S, const Eval &ev, const ArticulatedArgs &a) {
  const fiesta_hip_articulated_result &r = *a.res;
  if (a.dev) return artic_enqueue(st, S.tmp, ev, a, a.frame_poses, r);
  const size_t n = (size_t)a.n_configs, K = (size_t)a.n_spheres, F = (size_t)a.n_frames;
  Staging in{S.in, st}, out{S.out, st};
  const auto poses = in.add(a.frame_poses, 7 * n * F);
  in.alloc(), in.up(poses, 7 * n * F);
  const auto min_clearance = out.add(r.min_clearance, n);
  const auto min_sphere = out.add(r.min_sphere, n);
  const auto min_pos = out.add(r.min_pos, 3 * n), min_grad = out.add(r.min_grad, 3 * n);
  const auto n_below = out.add(r.n_below, n);
  const auto cost = out.add(r.cost, n);
  const auto frame_clearance = out.add(r.frame_clearance, n * F), frame_cost = out.add(r.frame_cost, n * F);
  const auto frame_grad = out.add(r.frame_grad, 6 * n * F), sphere_clearance = out.add(r.sphere_clearance, n * K);
  out.alloc();
  const fiesta_hip_articulated_result d{out.dev(min_clearance),   out.dev(min_sphere), out.dev(min_pos),    out.dev(min_grad),
                                        out.dev(n_below),         out.dev(cost),       out.dev(frame_clearance), out.dev(frame_cost),
                                        out.dev(frame_grad),      out.dev(sphere_clearance)};
  artic_enqueue(st, S.tmp, ev, a, in.dev(poses), d);
  out.back(min_clearance, n), out.back(min_sphere, n), out.back(min_pos, 3 * n), out.back(min_grad, 3 * n), out.back(n_below, n);
  out.back(cost, n), out.back(frame_clearance, n * F), out.back(frame_cost, n * F), out.back(frame_grad, 6 * n * F);
  out.back(sphere_clearance, n * K);
  FIESTA_HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace
}  // namespace fiesta
