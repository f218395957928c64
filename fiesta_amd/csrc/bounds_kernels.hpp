// fiesta_amd/csrc/bounds_kernels.hpp -- corridor bounds: fiesta_hip_corridor_bounds / _dev (include/fiesta_hip.h).
//
// The link between fiesta_hip_path_corridor and fiesta_hip_path_refine: per waypoint of a voxel polyline the box it may move in --
// its corridor box, intersected with the next one where the path changes boxes -- and per path whether the corridor is whole.  It
// reads no voxel: a pure function of the path batch and the corridor arrays, so corridor_bounds_run serves both stores (planner.hip).
//   k_path_check       path_kernels.hpp, unchanged (device variant only): waypoint offsets against the CSR rules
//   k_bounds_fill      bounds = NaN, box = -1 over all n_waypoints rows: rows that no valid path owns are deterministic
//   k_corridor_bounds  one wave per path (four paths per work-group, the 2-D grid of k_refine), lanes on consecutive waypoints in
//                      chunks of 64.  Per chunk: lane i loads w_i and w_{i+1}, the step lengths |w_{i+1} - w_i|_1 are scanned over
//                      the wave (int64, a carry between chunks) into the chain index c_i; b(i) is a binary search in the path's
//                      `entry` range; b(i + 1) comes from lane i + 1, and for the chunk's last lane from a search of its own for
//                      c_{i+1}; the flags of rules 3 and 4 are reduced by a ballot.
//                      `ok` is known only after the whole path: the rows are written as for an ok path while none of the flags is
//                      up, and a path that turns out not to be ok (rare: a skipped box, a first waypoint outside box 1) takes a
//                      second pass that writes its plain (or NaN) rows over them -- the same lane writes the same row both times.
// Every loop is bounded by the path's length or the logarithm of its box count.  No atomics, no cooperative launch, no LDS, no
// barrier, no wave waits for another.  Whatever the arrays hold, every index stays inside [o0, o1) and [b0, b1), both checked
// against n_waypoints and n_boxes.
#pragma once
#include "path_kernels.hpp"

namespace fiesta {
namespace {  // (planner.hip alone includes this header; the namespace is part of the kernels' symbol names)

constexpr int64_t kBoundsGridX = 1 << 15;  // work-groups per grid row
constexpr int kBoundsWaves = 4;            // paths per work-group
constexpr int kBoundsFillBlocks = 2048;

__global__ __launch_bounds__(256) void k_bounds_fill(double *bounds, int64_t *box, int64_t n_wp) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const double nan = NAN;
  if (bounds)
    for (int64_t i = t; i < 6 * n_wp; i += stride) bounds[i] = nan;
  if (box)
    for (int64_t i = t; i < n_wp; i += stride) box[i] = -1;
}

// the last k in [0, nb) with e[k] <= c (e non-decreasing), 0 if there is none: always a valid index
__device__ inline int64_t bounds_search(const int32_t *e, int64_t nb, long long c) {
  int64_t lo = 0, hi = nb;  // (the number of entries <= c lies in [lo, hi])
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((long long)e[mid] <= c)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo > 0 ? lo - 1 : 0;
}

__global__ __launch_bounds__(64 * kBoundsWaves) void k_corridor_bounds(const int32_t *w, const int64_t *off, const int64_t *nsamp, const int64_t *rng,
                                                                       int checked, int64_t n_paths, const int64_t *boff, const int32_t *boxes,
                                                                       const double *pos, const int32_t *entry, const int32_t *status,
                                                                       int64_t n_boxes, double inset, int void_broken, fiesta_hip_bounds_result r) {
  const int lane = threadIdx.x & 63;
  const int64_t p = ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * kBoundsWaves + (threadIdx.x >> 6);
  if (p >= n_paths) return;  // (uniform in the wave, and no barrier follows)
  const bool flagged = checked && nsamp[p] < 0;  // waypoint offsets out of order or out of range (k_path_check)
  const int64_t b0 = boff[p], b1 = boff[p + 1];
  if (flagged || b0 < 0 || b1 < b0 || b1 > n_boxes) {  // reads nothing, owns no row
    if (lane == 0 && r.ok) r.ok[p] = 0;
    return;
  }
  const int64_t o0 = checked ? rng[2 * p] : off[p], o1 = checked ? rng[2 * p + 1] : off[p + 1];
  const int64_t m = o1 - o0, nb = b1 - b0;
  const bool ok0 = status[p] == FIESTA_HIP_CORRIDOR_OK;
  bool ok = ok0;
  if (m > 0 && nb > 0) {  // (else: no row, or NaN rows and box -1, which the fill wrote)
    const int32_t *pw = w + 3 * o0, *pe = entry + b0;
    const double nan = NAN;
    for (int pass = 0; pass < 2; ++pass) {
      // pass 0 believes `ok0`; pass 1 runs only for a path that pass 0 found broken, and writes what a broken path gets
      const bool inter = pass == 0 && ok0, blank = void_broken && !inter;
      long long carry = 0;  // the chain index of the chunk's first waypoint
      int bad = 0;
      for (int64_t c0 = 0; c0 < m; c0 += 64) {
        const int64_t i = c0 + lane;
        const bool in = i < m, has_next = i + 1 < m;
        long long x = 0, y = 0, z = 0, dn = 0;
        if (in) x = pw[3 * i], y = pw[3 * i + 1], z = pw[3 * i + 2];
        if (has_next) {
          const long long dx = (long long)pw[3 * i + 3] - x, dy = (long long)pw[3 * i + 4] - y, dz = (long long)pw[3 * i + 5] - z;
          dn = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy) + (dz < 0 ? -dz : dz);
        }
        const long long incl = wave_inclusive_sum(dn);
        const long long c = carry + incl - dn;  // c_i
        carry += __shfl(incl, 63, 64);
        const long long b = in ? (long long)bounds_search(pe, nb, c) : 0;
        long long bn = __shfl_down(b, 1, 64);
        if (lane == 63 && has_next) bn = (long long)bounds_search(pe, nb, c + dn);  // (the next chunk's first waypoint)
        if (!has_next) bn = b;
        const bool change = bn == b + 1;
        int lane_bad = in && bn > b + 1;
        if (i == 0 && change) {  // rule 4: the first waypoint never moves, so it must lie in the box its successor changes to
          const int32_t *q = boxes + 6 * (b0 + bn);
          lane_bad |= x < q[0] || x > q[3] || y < q[1] || y > q[4] || z < q[2] || z > q[5];
        }
        bad |= __any(lane_bad);
        if (in) {
          if (r.bounds && !(pass == 0 && blank)) {  // (a void path's rows are the fill's NaN already)
            double *row = r.bounds + 6 * (o0 + i);
            if (blank) {
              for (int k = 0; k < 6; ++k) row[k] = nan;
            } else {
              const double *a = pos + 6 * (b0 + b);
              double v[6];
              for (int k = 0; k < 6; ++k) v[k] = a[k];
              if (inter && change) {
                const double *n = a + 6;
                for (int k = 0; k < 3; ++k) v[k] = v[k] > n[k] ? v[k] : n[k];
                for (int k = 3; k < 6; ++k) v[k] = v[k] < n[k] ? v[k] : n[k];
              }
              for (int k = 3; k < 6; ++k) v[k] = v[k] - inset;
              for (int k = 0; k < 6; ++k) row[k] = v[k];
            }
          }
          if (pass == 0 && r.box) r.box[o0 + i] = b0 + b;
        }
      }
      if (bad) ok = false;
      if (!(ok0 && bad)) break;  // (uniform: `bad` is a ballot's result)
    }
  }
  if (lane == 0 && r.ok) r.ok[p] = ok ? 1 : 0;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
// The device pipeline: fill, offset check (device batches), one launch.  Every pointer of `a` and `r` is a device pointer; tmp is
// the map's grow-only scratch.  Nothing is read back.
inline void corridor_bounds_launch(hipStream_t st, DevBuf<unsigned char> &tmp, const CorridorBoundsArgs &a, const fiesta_hip_bounds_result &r,
                                   bool checked) {
  int64_t *nsamp = nullptr, *rng = nullptr;
  if (checked) {
    tmp.ensure((size_t)a.n_paths * 24, st);
    nsamp = (int64_t *)tmp.p, rng = (int64_t *)(tmp.p + (size_t)a.n_paths * 8);
  }
  if (a.n_wp > 0 && (r.bounds || r.box)) {
    const int64_t blocks = std::min<int64_t>(kBoundsFillBlocks, (6 * a.n_wp + 255) / 256);
    hipLaunchKernelGGL(k_bounds_fill, dim3((unsigned)blocks), dim3(256), 0, st, r.bounds, r.box, a.n_wp);
  }
  if (checked) hipLaunchKernelGGL(k_path_check, dim3(1), dim3(1024), 0, st, a.off, a.n_paths, a.n_wp, nsamp, rng);
  const int64_t groups = (a.n_paths + kBoundsWaves - 1) / kBoundsWaves;
  const dim3 grid((unsigned)std::min<int64_t>(groups, kBoundsGridX), (unsigned)((groups + kBoundsGridX - 1) / kBoundsGridX));
  hipLaunchKernelGGL(k_corridor_bounds, grid, dim3(64 * kBoundsWaves), 0, st, a.w, a.off, (const int64_t *)nsamp, (const int64_t *)rng,
                     checked ? 1 : 0, a.n_paths, a.box_off, a.boxes, a.boxes_pos, a.entry, a.status, a.n_boxes, a.inset,
                     (a.flags & FIESTA_HIP_BOUNDS_VOID_BROKEN) ? 1 : 0, r);
  FIESTA_HIP_CHECK(hipGetLastError());
}

// Both variants of the call on a map's stream (n_paths > 0).  Host variant: the inputs are staged into S.in, the requested outputs
// come back through S.out, then the stream is synchronised.  Device variant: only enqueued.
inline void corridor_bounds_run(hipStream_t st, PlannerScratch &S, const CorridorBoundsArgs &a) {
  const fiesta_hip_bounds_result &r = *a.res;
  if (a.dev) {
    corridor_bounds_launch(st, S.tmp, a, r, true);
    return;
  }
  const size_t n = (size_t)a.n_paths, nw = (size_t)a.n_wp, nb = (size_t)a.n_boxes;
  Staging in{S.in, st}, out{S.out, st};
  const auto w = in.add(a.w, 3 * nw);
  const auto off = in.add(a.off, n + 1), box_off = in.add(a.box_off, n + 1);
  const auto boxes = in.add(a.boxes, 6 * nb);
  const auto boxes_pos = in.add(a.boxes_pos, 6 * nb);
  const auto entry = in.add(a.entry, nb), status = in.add(a.status, n);
  in.alloc();
  in.up(w, 3 * nw), in.up(off, n + 1), in.up(box_off, n + 1), in.up(boxes, 6 * nb), in.up(boxes_pos, 6 * nb), in.up(entry, nb), in.up(status, n);
  const auto bounds = out.add(r.bounds, 6 * nw);
  const auto box = out.add(r.box, nw);
  const auto ok = out.add(r.ok, n);
  out.alloc();
  CorridorBoundsArgs d = a;
  d.w = in.dev(w), d.off = in.dev(off), d.box_off = in.dev(box_off), d.boxes = in.dev(boxes), d.boxes_pos = in.dev(boxes_pos);
  d.entry = in.dev(entry), d.status = in.dev(status);
  const fiesta_hip_bounds_result dr{out.dev(bounds), out.dev(ok), out.dev(box)};
  corridor_bounds_launch(st, S.tmp, d, dr, false);
  out.back(bounds, 6 * nw), out.back(ok, n), out.back(box, nw);
  FIESTA_HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace
}  // namespace fiesta
