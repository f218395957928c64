// fiesta_amd/csrc/body_kernels.hpp -- body queries: a sphere-set robot body checked at batched poses: fiesta_hip_body_query / _dev
// (include/fiesta_hip.h).
//
// A sampling planner asks whether a body that is not round touches anything at a candidate pose, how close it is and where; an
// optimiser that models the body as spheres needs the summed obstacle penalty of a pose and its derivative with respect to the pose
// (a force and a torque).  Through the point queries that is K sphere centres per pose moved to the map and value + gradient of
// every one moved back (>= 56 B per sphere), then the penalty, the cross products and two reductions per pose on the caller's side.
// Here a sphere's (d, grad d) is the path calls' evaluator -- the point query bit for bit -- and one minimum and seven sums per pose
// leave the chip.
//   k_body_eval   persistent grid, a TEAM of T lanes per pose (T: the smallest power of two >= n_spheres, at most 64; 64 / T poses per
//                 wave, 256 / T per work-group and trip).  The sphere table lies once per work-group in LDS, one array per
//                 component, so the lanes of a team read consecutive doubles.  Every lane builds its pose's rotation; lane t takes
//                 spheres t, t + T, ... in a loop whose trip count is n_spheres' alone, evaluates value AND gradient once, keeps its
//                 own minimum (s, i), its count below the margin and seven partial sums (terms added in sphere order).  The team
//                 reduction is the xor butterfly of wave_reduce over offsets T/2 .. 1: both partners compute the same value, every
//                 lane of the team ends with the same bits.  The team's first lane stores the pose's outputs, the lane that owns the
//                 minimum's sphere its position and gradient, and every lane the clearances of its own spheres (consecutive lanes,
//                 consecutive doubles of a row).
// No floating-point atomics, no scratch buffer, no second kernel.  The order of every sum follows from T and n_spheres alone: the
// bits of a pose's outputs depend neither on n_poses, nor on the pose's place in the batch, nor on the grid.
#pragma once
#include <cstring>
#include <vector>

#include "path_cost_kernels.hpp"

namespace fiesta {
namespace {  // (planner.hip alone includes this header; the namespace is part of the kernels' symbol names)

constexpr int kBodyBlocks = 1024;  // persistent grid of k_body_eval: 4 work-groups of 4 waves per CU (4 x 32 KiB of LDS at 1024 spheres)

// the team size of a table of k spheres, as a shift: the smallest power of two >= k, at most 64
inline int body_team_shift(int k) {
  int s = 0;
  while (s < 6 && (1 << s) < k) ++s;
  return s;
}

// sph: the table as the caller gave it (cx, cy, cz, r per sphere), on the device.  Dynamic LDS: 4 * K doubles.  rp: the result struct
// on the device, behind the table: its eight pointers are read where they are used (as kernel arguments they stay in scalar
// registers across the sphere loop, next to the evaluator's geometry, and spill)
template <class Eval>
__global__ __launch_bounds__(256) void k_body_eval(Eval ev, const double *sph, int K, int shift, const double *poses, int64_t n_poses,
                                                   double margin, const fiesta_hip_body_result *rp) {
  extern __shared__ double body_tab[];  // cx[K], cy[K], cz[K], r[K]
  for (int i = threadIdx.x; i < 4 * K; i += 256) body_tab[(i & 3) * K + (i >> 2)] = sph[i];
  __syncthreads();
  const int T = 1 << shift, t = threadIdx.x & (T - 1), per = 256 >> shift;
  const int64_t groups = (n_poses + per - 1) / per;
  for (int64_t grp = blockIdx.x; grp < groups; grp += gridDim.x) {  // (uniform in the work-group)
    const int64_t p = grp * per + (threadIdx.x >> shift);
    const bool have = p < n_poses;
    double q[7] = {0, 0, 0, 1, 0, 0, 0};
    if (have) {
#pragma unroll
      for (int c = 0; c < 7; ++c) q[c] = poses[7 * p + c];
    }
    const double qw = q[3], qx = q[4], qy = q[5], qz = q[6];
    const double s = ((qw * qw + qx * qx) + qy * qy) + qz * qz;
    const double k = 2.0 / s;
    bool valid = have && s > 0 && __builtin_isfinite(k);
#pragma unroll
    for (int c = 0; c < 7; ++c) valid = valid && __builtin_isfinite(q[c]);
    const double xx = qx * qx, yy = qy * qy, zz = qz * qz, xy = qx * qy, xz = qx * qz, yz = qy * qz, wx = qw * qx, wy = qw * qy, wz = qw * qz;
    const double R[3][3] = {{1.0 - k * (yy + zz), k * (xy - wz), k * (xz + wy)},
                            {k * (xy + wz), 1.0 - k * (xx + zz), k * (yz - wx)},
                            {k * (xz - wy), k * (yz + wx), 1.0 - k * (xx + yy)}};
    double bv = INFINITY, bx[3] = {NAN, NAN, NAN}, bg[3] = {NAN, NAN, NAN};  // this lane's minimum: (value, index), smaller value, then smaller index
    int bi = INT_MAX, nb = 0;
    double acc[7] = {0, 0, 0, 0, 0, 0, 0};
    double *const clearance = rp->sphere_clearance;
    for (int i0 = 0; i0 < K; i0 += T) {  // (uniform: a lane past the table or of an invalid pose contributes the identity)
      const int i = i0 + t;
      if (valid && i < K) {
        const double cx = body_tab[i], cy = body_tab[K + i], cz = body_tab[2 * K + i], rad = body_tab[3 * K + i];
        double a[3], x[3], g[3], phi, gam[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          a[c] = (R[c][0] * cx + R[c][1] * cy) + R[c][2] * cz;
          x[c] = q[c] + a[c];
        }
        const double d = ev(x, g);
        const double si = d - rad;
        nb += cost_penalty(si, g, margin, &phi, gam);
        acc[0] += phi;
        acc[1] += gam[0], acc[2] += gam[1], acc[3] += gam[2];
        acc[4] += a[1] * gam[2] - a[2] * gam[1];
        acc[5] += a[2] * gam[0] - a[0] * gam[2];
        acc[6] += a[0] * gam[1] - a[1] * gam[0];
        if (si < bv) {  // (this lane's indices only grow)
          bv = si, bi = i;
#pragma unroll
          for (int c = 0; c < 3; ++c) bx[c] = x[c], bg[c] = g[c];
        }
        if (clearance) clearance[p * K + i] = si;
      }
    }
    for (int o = T >> 1; o > 0; o >>= 1) {  // wave_reduce's butterfly, limited to the team
#pragma unroll
      for (int c = 0; c < 7; ++c) acc[c] = acc[c] + __shfl_xor(acc[c], o, 64);
      nb += __shfl_xor(nb, o, 64);
      const double ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov < bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
    }
    if (!have) continue;
    const fiesta_hip_body_result r = *rp;
    if (valid) {
      if (t == 0) {
        if (r.min_clearance) r.min_clearance[p] = bv;
        if (r.min_sphere) r.min_sphere[p] = bi;
        if (r.n_below) r.n_below[p] = nb;
        if (r.cost) r.cost[p] = acc[0];
        if (r.grad) {
#pragma unroll
          for (int c = 0; c < 6; ++c) r.grad[6 * p + c] = acc[1 + c];
        }
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
        for (int c = 0; c < 6; ++c)
          if (r.grad) r.grad[6 * p + c] = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          if (r.min_pos) r.min_pos[3 * p + c] = NAN;
          if (r.min_grad) r.min_grad[3 * p + c] = NAN;
        }
      }
      if (r.sphere_clearance)
        for (int i = t; i < K; i += T) r.sphere_clearance[p * K + i] = NAN;
    }
  }
}

// The call's header in the map's scratch -- the sphere table, then the result struct `r` of device pointers -- and the launch.  One
// copy on the stream from a block of pageable host memory: it has left the host when the copy call returns.
template <class Eval>
void body_enqueue(hipStream_t st, DevBuf<unsigned char> &tmp, const Eval &ev, const BodyArgs &a, const double *poses, const fiesta_hip_body_result &r) {
  const int K = a.n_spheres, shift = body_team_shift(K), per = 256 >> shift;
  const size_t tab = (size_t)K * 4 * sizeof(double);
  const unsigned grid = (unsigned)std::min<int64_t>((a.n_poses + per - 1) / per, kBodyBlocks);
  std::vector<unsigned char> head(tab + sizeof(r));
  memcpy(head.data(), a.spheres, tab), memcpy(head.data() + tab, &r, sizeof(r));
  tmp.ensure(head.size(), st);
  FIESTA_HIP_CHECK(hipMemcpyAsync(tmp.p, head.data(), head.size(), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_body_eval<Eval>, dim3(grid), dim3(256), tab, st, ev, (const double *)tmp.p, K, shift, poses, a.n_poses, a.margin,
                     (const fiesta_hip_body_result *)(tmp.p + tab));
  FIESTA_HIP_CHECK(hipGetLastError());
}

// Both variants of the call on a map's stream.  The device variant only enqueues; the host variant stages the poses through S.in
// and every output through S.out, synchronises and copies back.  It always runs on the device.
template <class Eval>
void body_query_run(hipStream_t st, PlannerScratch &S, const Eval &ev, const BodyArgs &a) {
  const fiesta_hip_body_result &r = *a.res;
  if (a.dev) return body_enqueue(st, S.tmp, ev, a, a.poses, r);
  const size_t n = (size_t)a.n_poses, K = (size_t)a.n_spheres;
  Staging in{S.in, st}, out{S.out, st};
  const auto poses = in.add(a.poses, 7 * n);
  in.alloc(), in.up(poses, 7 * n);
  const auto min_clearance = out.add(r.min_clearance, n);
  const auto min_sphere = out.add(r.min_sphere, n);
  const auto min_pos = out.add(r.min_pos, 3 * n), min_grad = out.add(r.min_grad, 3 * n);
  const auto n_below = out.add(r.n_below, n);
  const auto cost = out.add(r.cost, n), grad = out.add(r.grad, 6 * n), sphere_clearance = out.add(r.sphere_clearance, n * K);
  out.alloc();
  const fiesta_hip_body_result d{out.dev(min_clearance), out.dev(min_sphere), out.dev(min_pos), out.dev(min_grad),
                                 out.dev(n_below),       out.dev(cost),       out.dev(grad),    out.dev(sphere_clearance)};
  body_enqueue(st, S.tmp, ev, a, in.dev(poses), d);
  out.back(min_clearance, n), out.back(min_sphere, n), out.back(min_pos, 3 * n), out.back(min_grad, 3 * n), out.back(n_below, n);
  out.back(cost, n), out.back(grad, 6 * n), out.back(sphere_clearance, n * K);
  FIESTA_HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace
}  // namespace fiesta
