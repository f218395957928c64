// fiesta_amd/csrc/reach_path_kernels.hpp -- paths out of a cost-to-go field: fiesta_hip_reach_paths / _dev (include/fiesta_hip.h).
//
// fiesta_hip_reach_field tells a planner which targets the robot can reach and at what cost; this call extracts the paths.  It reads
// nothing of a map but a cost field (the map's retained scratch field or the caller's array), the box it covers, and the map's
// resolution and origin.  Per target: the DESCENT from the target down the field to a seed (the first move, in reach_model's move
// order, whose voxel costs exactly the move's weight less), and -- with FIESTA_HIP_REACH_PATHS_SHORTCUT -- the greedy line-of-sight
// anchors over it (string pulling through the field's own traversable set, by the ray cast's traversal: ray_walk.hpp).
// Two passes over the same device function, no data-dependent allocation:
//   k_reach_path_count<CONN, SHORTCUT>  per target: status, number of moves, number of waypoints (into offsets[p + 1])
//   k_reach_path_scan                   offsets[1 .. n] -> running totals, offsets[0] = 0: one work-group striding with a carry
//   k_reach_path_write<CONN, SHORTCUT>  redoes the rule and stores waypoint k of a path of c at offsets[p] + (c - 1 - k) -- seed first,
//                                       target last -- if that index lies below the capacity
// Raw mode (reach_path_raw): one lane per target, grid-stride; a step issues its 6 or 26 neighbour loads together and takes the
//   first match in move order.
// Shortcut mode (reach_path_wave): one wave per target.  A descent step is one load per lane (lane m holds move m) and a ballot.
//   The wave keeps the next 64 voxels of the descent, one per lane, IN REGISTERS (a window that a shuffle moves along: no LDS and
//   nothing to synchronise); every lane walks anchor -> its own voxel with dda_walk, a ballot of the failures and a find-first give
//   the next anchor; lanes past max_span or past the descent's end count as failures.  A window without failure moves on whole.
// Every value is an integer (positions: one f64 expression per coordinate); both modes follow the same sequential rule, so the
// outputs do not depend on the mode's shape, the grid or the scheduling.  No atomics, no LDS in the path kernels, no scratch.
#pragma once
#include <algorithm>
#include <climits>

#include "../../include/fiesta_hip.h"
#include "common.hpp"
#include "planner.hpp"
#include "planner_args.hpp"
#include "ray_walk.hpp"
#include "wave_ops.hpp"

namespace fiesta {
namespace {  // (planner.hip alone includes this header; the namespace is part of the kernels' symbol names)

constexpr int64_t kReachPathMaxVoxels = 1ll << 28;  // of an explicit box (reach_field's bound)
constexpr int kReachPathManhattan = 4095;           // voxel steps between the ends of a visibility test (the ray query's bound)
constexpr int kReachPathBlock = 256, kReachPathMaxBlocks = 2048;

struct ReachPathField {
  const int32_t *cost;  // ex * ey * ez, box-local order
  int ox, oy, oz;       // map voxel of box voxel (0, 0, 0)
  int ex, ey, ez;
  double res, org[3];   // Vox2Pos
};
struct ReachPathOut {  // device pointers; offsets is never null
  int64_t *offsets;
  int32_t *vox;
  double *pos;
  int32_t *status, *n_moves;
  int64_t capacity;
};

__device__ inline bool reach_path_in(const ReachPathField &f, int x, int y, int z) {
  return (unsigned)x < (unsigned)f.ex && (unsigned)y < (unsigned)f.ey && (unsigned)z < (unsigned)f.ez;
}
__device__ inline int reach_path_cost(const ReachPathField &f, int x, int y, int z) { return f.cost[((int64_t)x * f.ey + y) * f.ez + z]; }

// move m of reach_model.reach_moves(CONN) as an index into the 27 (dx, dy, dz) triples in lexicographic order (13: no move)
template <int CONN>
__device__ inline int reach_path_move(int m) {
  if (CONN == 26) return m < 13 ? m : m + 1;
  return (int)((0x16100E0C0A04ull >> (8 * m)) & 0xFFu);  // 4, 10, 12, 14, 16, 22: one axis changed
}

// the target's own voxel and cost: status, and (OK only) the box-local voxel and its cost
__device__ inline int reach_path_start(const ReachPathField &f, const int32_t *targets, int64_t p, int &x, int &y, int &z, int &c) {
  const int64_t lx = (int64_t)targets[3 * p] - f.ox, ly = (int64_t)targets[3 * p + 1] - f.oy, lz = (int64_t)targets[3 * p + 2] - f.oz;
  if (lx < 0 || lx >= f.ex || ly < 0 || ly >= f.ey || lz < 0 || lz >= f.ez) return FIESTA_HIP_REACH_PATH_OUTSIDE;
  x = (int)lx, y = (int)ly, z = (int)lz;
  c = reach_path_cost(f, x, y, z);
  if (c == -1) return FIESTA_HIP_REACH_PATH_BLOCKED;
  if (c == INT32_MAX) return FIESTA_HIP_REACH_PATH_UNREACHED;
  return c < -1 ? FIESTA_HIP_REACH_PATH_BROKEN : FIESTA_HIP_REACH_PATH_OK;
}

// waypoint k (0: the target) of path p, whose waypoints start at `first` and number `count`: the path is stored seed first
__device__ inline void reach_path_store(const ReachPathField &f, const ReachPathOut &o, int64_t first, int64_t count, int64_t k, int x, int y,
                                        int z) {
  const int64_t at = first + (count - 1 - k);
  if (k >= count || at >= o.capacity) return;  // (k >= count: the field changed between the two passes -- never below `first`)
  const int vx = f.ox + x, vy = f.oy + y, vz = f.oz + z;
  if (o.vox) o.vox[3 * at] = vx, o.vox[3 * at + 1] = vy, o.vox[3 * at + 2] = vz;
  if (o.pos) {
    o.pos[3 * at] = ((double)vx + 0.5) * f.res + f.org[0];
    o.pos[3 * at + 1] = ((double)vy + 0.5) * f.res + f.org[1];
    o.pos[3 * at + 2] = ((double)vz + 0.5) * f.res + f.org[2];
  }
}

// Raw mode, one lane: every voxel of the descent is a waypoint.  WRITE: `first` / `count` from the scanned offsets (count > 0: the
// count pass found the path whole).  Returns the status; L = number of moves.  Every step lowers the cost by at least 3 and only
// costs >= 0 are followed, so the loop ends after at most cost / 3 steps whatever the array holds; no read leaves the box.
template <int CONN, bool WRITE>
__device__ inline int reach_path_raw(const ReachPathField &f, const ReachPathOut &o, const int32_t *targets, int64_t p, int64_t first, int64_t count,
                                     int &L) {
  int x = 0, y = 0, z = 0, c = 0;
  L = -1;
  const int st = reach_path_start(f, targets, p, x, y, z, c);
  if (st != FIESTA_HIP_REACH_PATH_OK) return st;
  int k = 0;
  if (WRITE) reach_path_store(f, o, first, count, 0, x, y, z);
  while (c > 0) {
    int nc[27];  // (indexed by constants only: registers)
#pragma unroll
    for (int d = 0; d < 27; ++d) {
      const int dx = d / 9 - 1, dy = (d / 3) % 3 - 1, dz = d % 3 - 1, ch = (dx != 0) + (dy != 0) + (dz != 0);
      nc[d] = -1;
      if (ch == 0 || (CONN == 6 && ch != 1)) continue;
      if (reach_path_in(f, x + dx, y + dy, z + dz)) nc[d] = reach_path_cost(f, x + dx, y + dy, z + dz);
    }
    int pick = -1;
    bool bad = false;
#pragma unroll
    for (int d = 26; d >= 0; --d) {  // backwards: the first match in move order is assigned last
      const int dx = d / 9 - 1, dy = (d / 3) % 3 - 1, dz = d % 3 - 1, ch = (dx != 0) + (dy != 0) + (dz != 0);
      if (ch == 0 || (CONN == 6 && ch != 1)) continue;
      bad = bad || nc[d] < -1;
      if (nc[d] >= 0 && nc[d] == c - (2 + ch)) pick = d;  // (c - w cannot overflow, cost + w could)
    }
    if (bad || pick < 0) return FIESTA_HIP_REACH_PATH_BROKEN;
    const int dx = pick / 9 - 1, dy = (pick / 3) % 3 - 1, dz = pick % 3 - 1;
    x += dx, y += dy, z += dz;
    c -= 2 + (dx != 0) + (dy != 0) + (dz != 0);
    ++k;
    if (WRITE) reach_path_store(f, o, first, count, k, x, y, z);
  }
  L = k;
  return FIESTA_HIP_REACH_PATH_OK;
}

// visible(a, b) for box-local voxels (include/fiesta_hip.h): the traversal runs in MAP voxel units from centre to centre
__device__ inline bool reach_path_visible(const ReachPathField &f, int ax, int ay, int az, int bx, int by, int bz) {
  if (abs(ax - bx) + abs(ay - by) + abs(az - bz) > kReachPathManhattan) return false;
  const double a[3] = {(double)(f.ox + ax) + 0.5, (double)(f.oy + ay) + 0.5, (double)(f.oz + az) + 0.5};
  const double b[3] = {(double)(f.ox + bx) + 0.5, (double)(f.oy + by) + 0.5, (double)(f.oz + bz) + 0.5};
  bool ok = true;
  dda_walk<false, false>(a, b, nullptr, nullptr, [&](int x, int y, int z, int, bool) -> bool {
    const int lx = x - f.ox, ly = y - f.oy, lz = z - f.oz;  // (between two voxels of the box: no overflow)
    ok = reach_path_in(f, lx, ly, lz) && reach_path_cost(f, lx, ly, lz) >= 0;
    return !ok;
  });
  return ok;
}

// Shortcut mode, one wave; every argument and every result is wave-uniform, `count` of the WRITE pass as in reach_path_raw.
// anchors: the number of waypoints.  The rule (include/fiesta_hip.h): from anchor D[i], j = i + 1; while j < L and j + 1 - i <= max_span
// and visible(D[i], D[j + 1]): ++j; the next anchor is D[j].  Here lane l of the window holds D[r0 + l]; it PASSES if r0 + l == i + 1
// (a legal move of the flood, never tested) or r0 + l <= L and r0 + l - i <= max_span and visible; with f the first lane that fails,
// j = r0 + f - 1.  No failure in 64 lanes: the same anchor goes on with the next 64 voxels.
template <int CONN, bool WRITE>
__device__ inline int reach_path_wave(const ReachPathField &f, const ReachPathOut &o, const int32_t *targets, int64_t p, int max_span, int64_t first,
                                      int64_t count, int &L, int &anchors) {
  const int lane = threadIdx.x & 63;
  int ax = 0, ay = 0, az = 0, c = 0;  // the anchor D[i]; below: the cost of the newest descent voxel
  L = -1, anchors = 0;
  const int st = reach_path_start(f, targets, p, ax, ay, az, c);
  if (st != FIESTA_HIP_REACH_PATH_OK) return st;
  if (WRITE && lane == 0) reach_path_store(f, o, first, count, 0, ax, ay, az);
  int k = 1;                             // anchors so far
  int i = 0, r0 = 1, t = 1;              // anchor index; index of the window's lane 0; number of descent voxels known (D[0 .. t - 1])
  int dx = ax, dy = ay, dz = az;         // D[t - 1]
  int lx = ax, ly = ay, lz = az;         // D[r0 - 1]: the last voxel accepted before the window
  int wx = 0, wy = 0, wz = 0;            // this lane's voxel of the window: D[r0 + lane], valid if r0 + lane < t
  // this lane's move of the descent step
  int mx = 0, my = 0, mz = 0, mw = 0;
  if (lane < CONN) {
    const int d = reach_path_move<CONN>(lane);
    mx = d / 9 - 1, my = (d / 3) % 3 - 1, mz = d % 3 - 1, mw = 2 + (mx != 0) + (my != 0) + (mz != 0);
  }
  while (true) {
    // fill the window: up to 64 voxels ahead of r0, or down to cost 0
    while (t < r0 + 64 && c > 0) {
      const int nx = dx + mx, ny = dy + my, nz = dz + mz;
      int nc = -1;
      if (lane < CONN && reach_path_in(f, nx, ny, nz)) nc = reach_path_cost(f, nx, ny, nz);
      const unsigned long long bad = __ballot(nc < -1), hit = __ballot(nc >= 0 && nc == c - mw);  // (lanes >= CONN: nc = -1, mw = 0)
      if (bad || !hit) return FIESTA_HIP_REACH_PATH_BROKEN;
      const int m = __ffsll((long long)hit) - 1;
      dx = __shfl(nx, m), dy = __shfl(ny, m), dz = __shfl(nz, m);
      c -= __shfl(mw, m);
      if (lane == t - r0) wx = dx, wy = dy, wz = dz;
      ++t;
    }
    if (c == 0 && i == t - 1) break;  // the anchor is the descent's last voxel
    const int idx = r0 + lane;
    bool pass = idx == i + 1;
    if (!pass && idx < t && idx - i <= max_span) pass = reach_path_visible(f, ax, ay, az, wx, wy, wz);
    const unsigned long long fail = __ballot(!pass);
    if (!fail) {  // (64 voxels, all visible; the descent goes on or the next window is empty and its lane 0 fails)
      lx = __shfl(wx, 63), ly = __shfl(wy, 63), lz = __shfl(wz, 63);
      r0 += 64;
      continue;
    }
    const int fl = __ffsll((long long)fail) - 1;  // j = r0 + fl - 1
    if (fl > 0) lx = __shfl(wx, fl - 1), ly = __shfl(wy, fl - 1), lz = __shfl(wz, fl - 1);
    ax = lx, ay = ly, az = lz;
    i = r0 + fl - 1;
    if (WRITE && lane == 0) reach_path_store(f, o, first, count, k, ax, ay, az);
    ++k;
    // the window moves on to D[i + 1 ..]: lane l takes what lane l + fl held
    wx = __shfl(wx, (lane + fl) & 63), wy = __shfl(wy, (lane + fl) & 63), wz = __shfl(wz, (lane + fl) & 63);
    r0 = i + 1;
  }
  L = t - 1;
  anchors = k;
  return FIESTA_HIP_REACH_PATH_OK;
}

// count pass: offsets[p + 1] = number of waypoints of path p (the scan turns them into totals)
template <int CONN, bool SHORTCUT>
__global__ __launch_bounds__(kReachPathBlock) void k_reach_path_count(ReachPathField f, ReachPathOut o, const int32_t *targets, int64_t n, int max_span) {
  const int64_t stride = (int64_t)gridDim.x * (SHORTCUT ? kReachPathBlock / 64 : kReachPathBlock);
  for (int64_t p = SHORTCUT ? blockIdx.x * (int64_t)(kReachPathBlock / 64) + (threadIdx.x >> 6) : blockIdx.x * (int64_t)kReachPathBlock + threadIdx.x;
       p < n; p += stride) {
    int L = -1, cnt = 0, st;
    if (SHORTCUT) {
      st = reach_path_wave<CONN, false>(f, o, targets, p, max_span, 0, 0, L, cnt);
    } else {
      st = reach_path_raw<CONN, false>(f, o, targets, p, 0, 0, L);
      cnt = L + 1;
    }
    if (st != FIESTA_HIP_REACH_PATH_OK) L = -1, cnt = 0;
    if (!SHORTCUT || (threadIdx.x & 63) == 0) {
      o.offsets[p + 1] = cnt;
      if (o.status) o.status[p] = st;
      if (o.n_moves) o.n_moves[p] = L;
    }
  }
}

// offsets[1 .. n]: counts -> inclusive running totals; offsets[0] = 0.  One work-group of 256, 256 entries per trip, the carry in a register.
__global__ __launch_bounds__(256) void k_reach_path_scan(int64_t *offsets, int64_t n) {
  __shared__ long long s_wave[4];
  if (threadIdx.x == 0) offsets[0] = 0;
  (void)block_scan_stride<1, 4>(
      n, s_wave, [&](int64_t i) { return (long long)offsets[1 + i]; },
      [&](int64_t i, long long before, long long v) { offsets[1 + i] = (int64_t)(before + v); });
}

template <int CONN, bool SHORTCUT>
__global__ __launch_bounds__(kReachPathBlock) void k_reach_path_write(ReachPathField f, ReachPathOut o, const int32_t *targets, int64_t n, int max_span) {
  const int64_t stride = (int64_t)gridDim.x * (SHORTCUT ? kReachPathBlock / 64 : kReachPathBlock);
  for (int64_t p = SHORTCUT ? blockIdx.x * (int64_t)(kReachPathBlock / 64) + (threadIdx.x >> 6) : blockIdx.x * (int64_t)kReachPathBlock + threadIdx.x;
       p < n; p += stride) {
    const int64_t first = o.offsets[p], count = o.offsets[p + 1] - first;
    if (count <= 0 || first >= o.capacity) continue;  // no path, or all of it beyond the capacity
    int L, cnt;
    if (SHORTCUT)
      (void)reach_path_wave<CONN, true>(f, o, targets, p, max_span, first, count, L, cnt);
    else
      (void)reach_path_raw<CONN, true>(f, o, targets, p, first, count, L);
  }
}

template <int CONN, bool SHORTCUT>
void reach_path_passes(hipStream_t st, const ReachPathField &f, const ReachPathOut &o, const int32_t *targets, int64_t n, int max_span, bool count) {
  const int per = SHORTCUT ? kReachPathBlock / 64 : kReachPathBlock;
  const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((n + per - 1) / per, kReachPathMaxBlocks));
  if (count)
    hipLaunchKernelGGL((k_reach_path_count<CONN, SHORTCUT>), dim3(blocks), dim3(kReachPathBlock), 0, st, f, o, targets, n, max_span);
  else
    hipLaunchKernelGGL((k_reach_path_write<CONN, SHORTCUT>), dim3(blocks), dim3(kReachPathBlock), 0, st, f, o, targets, n, max_span);
  FIESTA_HIP_CHECK(hipGetLastError());
}

inline void reach_path_launch(hipStream_t st, const ReachPathField &f, const ReachPathOut &o, const int32_t *targets, int64_t n, int connectivity,
                              bool shortcut, int max_span, bool count) {
  if (connectivity == 6) {
    if (shortcut)
      reach_path_passes<6, true>(st, f, o, targets, n, max_span, count);
    else
      reach_path_passes<6, false>(st, f, o, targets, n, max_span, count);
  } else {
    if (shortcut)
      reach_path_passes<26, true>(st, f, o, targets, n, max_span, count);
    else
      reach_path_passes<26, false>(st, f, o, targets, n, max_span, count);
  }
}

// Both variants of the call on a map's stream; res / org: the map's resolution and origin -- nothing else of a map is read, so
// both stores share this function.  The device variant only enqueues (count, scan, write).  The host variant stages the targets
// through P.in and the outputs through P.out, reads the totals back between the count and the write pass -- so that it stages
// min(total, capacity) waypoints, not the capacity -- and synchronises.
inline void reach_paths_run(hipStream_t st, PlannerScratch &P, double res, const double *org, const ReachPathArgs &a) {
  ReachScratch &S = P.reach;
  const fiesta_hip_reach_paths_result &r = *a.res;
  ReachPathField f{};
  if (a.cost) {
    f.ox = a.box_lo[0], f.oy = a.box_lo[1], f.oz = a.box_lo[2];  // (the extents are checked: each at most 2^28)
    f.ex = (int)((int64_t)a.box_hi[0] - a.box_lo[0] + 1), f.ey = (int)((int64_t)a.box_hi[1] - a.box_lo[1] + 1);
    f.ez = (int)((int64_t)a.box_hi[2] - a.box_lo[2] + 1);
    const int64_t nvox = (int64_t)f.ex * f.ey * f.ez;
    if (a.dev) {
      f.cost = a.cost;
    } else {  // the caller's field becomes the retained one
      S.field_valid = false;
      S.cost.ensure_exact((size_t)nvox, st);
      FIESTA_HIP_CHECK(hipMemcpyAsync(S.cost.p, a.cost, (size_t)nvox * sizeof(int32_t), hipMemcpyHostToDevice, st));
      for (int c = 0; c < 3; ++c) S.field_lo[c] = a.box_lo[c], S.field_hi[c] = a.box_hi[c];
      S.field_connectivity = a.connectivity;
      S.field_valid = true;
      f.cost = S.cost.p;
    }
  } else {
    if (!S.field_valid) throw Error(FIESTA_HIP_ERR_STATE, "reach_paths: the map retains no cost field (no reach_field call left one)");
    if (S.field_connectivity != a.connectivity)
      throw Error(FIESTA_HIP_ERR_INVALID, "reach_paths: connectivity differs from the retained field's");
    f.ox = S.field_lo[0], f.oy = S.field_lo[1], f.oz = S.field_lo[2];
    f.ex = S.field_hi[0] - S.field_lo[0] + 1, f.ey = S.field_hi[1] - S.field_lo[1] + 1, f.ez = S.field_hi[2] - S.field_lo[2] + 1;
    f.cost = S.cost.p;
  }
  f.res = res, f.org[0] = org[0], f.org[1] = org[1], f.org[2] = org[2];
  const bool shortcut = (a.flags & FIESTA_HIP_REACH_PATHS_SHORTCUT) != 0;
  const int64_t n = a.n_targets;
  if (a.dev) {
    const ReachPathOut o{r.offsets, r.waypoints_vox, r.waypoints_pos, r.status, r.n_moves, a.capacity};
    if (n > 0) reach_path_launch(st, f, o, a.targets, n, a.connectivity, shortcut, a.max_span, true);
    hipLaunchKernelGGL(k_reach_path_scan, dim3(1), dim3(256), 0, st, r.offsets, n);
    FIESTA_HIP_CHECK(hipGetLastError());
    if (n > 0 && a.capacity > 0 && (r.waypoints_vox || r.waypoints_pos)) reach_path_launch(st, f, o, a.targets, n, a.connectivity, shortcut, a.max_span, false);
    return;
  }
  if (n == 0) {
    r.offsets[0] = 0;
    FIESTA_HIP_CHECK(hipStreamSynchronize(st));  // (an uploaded field is in place when the call returns)
    return;
  }
  const size_t cnt = (size_t)n;
  Staging in{P.in, st}, out{P.out, st};
  const auto targets = in.add(a.targets, 3 * cnt);
  in.alloc(), in.up(targets, 3 * cnt);
  const int32_t *dt = in.dev(targets);
  // offsets, status and n_moves; the waypoints follow once their number is known
  const auto offsets = out.add(r.offsets, cnt + 1);
  const auto status = out.add(r.status, cnt), n_moves = out.add(r.n_moves, cnt);
  const size_t head = out.end;
  out.alloc();
  ReachPathOut o{out.dev(offsets), nullptr, nullptr, out.dev(status), out.dev(n_moves), 0};
  reach_path_launch(st, f, o, dt, n, a.connectivity, shortcut, a.max_span, true);
  hipLaunchKernelGGL(k_reach_path_scan, dim3(1), dim3(256), 0, st, o.offsets, n);
  FIESTA_HIP_CHECK(hipGetLastError());
  out.back(offsets, cnt + 1), out.back(status, cnt), out.back(n_moves, cnt);
  FIESTA_HIP_CHECK(hipStreamSynchronize(st));
  const int64_t w = std::min<int64_t>(r.offsets[n], a.capacity);
  if (w <= 0 || (!r.waypoints_vox && !r.waypoints_pos)) return;
  const auto pos = out.add(r.waypoints_pos, 3 * (size_t)w);
  const auto vox = out.add(r.waypoints_vox, 3 * (size_t)w);
  out.alloc(head);  // (the buffer may move; the scanned offsets are kept: the write pass reads them)
  o = ReachPathOut{out.dev(offsets), out.dev(vox), out.dev(pos), nullptr, nullptr, w};
  reach_path_launch(st, f, o, dt, n, a.connectivity, shortcut, a.max_span, false);
  out.back(pos, 3 * (size_t)w), out.back(vox, 3 * (size_t)w);
  FIESTA_HIP_CHECK(hipStreamSynchronize(st));
}

}  // namespace
}  // namespace fiesta
