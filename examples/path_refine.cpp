// examples/path_refine.cpp -- "and now make the paths flyable": the optimiser's step after the corridors, through the drop-in class
// (include/fiesta/ESDFMap.h), on the scene of examples/corridor.cpp -- 40 x 40 x 20 voxels (0.2 m) seen through one view cone from
// voxel (5, 20, 10) along +x that ends on a wall at x = 30 and holds one pillar.
//   GetFrontierVoxels, ReachField   where known free space ends, and the travel cost from the robot's voxel to all of it
//   ReachPaths                      the RAW paths to every frontier voxel: voxel staircases, one waypoint per move
//   PathCorridor                    per path the safe flight corridor: overlapping boxes of free space
//   (here)                          per waypoint the box it may move in: its corridor box, intersected with the next box where the
//                                   path changes boxes -- what fiesta_amd.corridor_bounds computes in Python
//   RefinePaths                     every path descends on obstacle cost + smoothness inside its boxes, the whole loop on the device
// Prints the longest path before and after, and one JSON line at the end; tests/test_cpp_refine.py builds the same scene through the
// Python class and asserts that the numbers agree.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fiesta/ESDFMap.h"

int main() {
  fiesta::ESDFMap m(Eigen::Vector3d(-4.0, -4.0, 0.0), 0.2, Eigen::Vector3d(8.0, 8.0, 4.0));  // 40 x 40 x 20 voxels
  m.SetParameters(0.70, 0.35, 0.12, 0.97, 0.80);
  m.SetOriginalRange();
  const int sx = 5, sy = 20, sz = 10, range2 = 28 * 28, wall = 30;
  for (int cycle = 0; cycle < 3; ++cycle) {  // (an obstacle needs three hits to count as occupied)
    for (int x = sx + 1; x <= wall; ++x)
      for (int y = 0; y < 40; ++y)
        for (int z = 0; z < 20; ++z) {
          const int dx = x - sx, dy = y - sy, dz = z - sz;
          if (dy * dy + dz * dz > dx * dx || dx * dx + dy * dy + dz * dz > range2) continue;  // outside the cone
          const bool hit = x == wall || (x == 18 && y >= 19 && y <= 21);
          if (cycle == 0 || hit) m.SetOccupancy(Eigen::Vector3i(x, y, z), hit ? 1 : 0);
        }
    if (cycle == 0)  // the pocket: 4 x 4 x 4 free voxels behind the wall
      for (int x = 33; x <= 36; ++x)
        for (int y = 18; y <= 21; ++y)
          for (int z = 8; z <= 11; ++z) m.SetOccupancy(Eigen::Vector3i(x, y, z), 0);
    m.UpdateOccupancy(true);
  }
  m.UpdateESDF();

  std::vector<Eigen::Vector3i> frontier;
  m.GetFrontierVoxels(0.0, frontier);
  std::sort(frontier.begin(), frontier.end(), [](const Eigen::Vector3i &a, const Eigen::Vector3i &b) {
    return a(0) != b(0) ? a(0) < b(0) : (a(1) != b(1) ? a(1) < b(1) : a(2) < b(2));
  });
  const std::vector<Eigen::Vector3i> robot{Eigen::Vector3i(sx + 7, sy, sz)};
  m.ReachField(nullptr, nullptr, robot, {}, 0.0, 26, 0, nullptr);
  const auto paths = m.ReachPaths(frontier, 26, false);
  const auto cor = m.PathCorridor(paths.vox, paths.offsets, 8);

  // per waypoint its box: the last box of its path entered at or before the waypoint's chain index; where the next waypoint lies in
  // the next box, the intersection of the two (consecutive boxes share a voxel).  A path is refined inside its corridor only if the
  // corridor is whole, no box is skipped between two waypoints and its first waypoint (which never moves) lies in its successor's box;
  // every other path keeps each waypoint's own box and is not counted as `ok`.  Every upper face is pulled in by 2^-20 of a voxel: it
  // is the lower face of the next voxel, and a waypoint clamped exactly onto it would be filed under that voxel.
  const size_t n = frontier.size();
  std::vector<double> bounds(2 * paths.pos.size(), 0.0);
  std::vector<char> ok(n, 0);
  for (size_t p = 0; p < n; ++p) {
    const int64_t o0 = paths.offsets[p], o1 = paths.offsets[p + 1], b0 = cor.offsets[p], b1 = cor.offsets[p + 1];
    ok[p] = cor.status[p] == FIESTA_HIP_CORRIDOR_OK;
    std::vector<int64_t> box((size_t)(o1 - o0), b0);
    int64_t chain = 0, b = b0;
    for (int64_t i = o0; i < o1; ++i) {
      if (i > o0)
        for (int c = 0; c < 3; ++c) chain += std::abs(paths.vox[3 * i + c] - paths.vox[3 * (i - 1) + c]);
      while (b + 1 < b1 && cor.entry[b + 1] <= chain) ++b;
      box[(size_t)(i - o0)] = b;
    }
    for (int64_t i = o0; i < o1; ++i) {
      double *row = &bounds[6 * i];
      if (b1 == b0) {  // no box at all: a row the refinement rejects (its path reports INVALID)
        for (int c = 0; c < 6; ++c) row[c] = std::nan("");
        continue;
      }
      const int64_t bi = box[(size_t)(i - o0)];
      for (int c = 0; c < 6; ++c) row[c] = cor.pos[6 * bi + c];
      if (i + 1 >= o1) continue;
      const int64_t bn = box[(size_t)(i + 1 - o0)];
      if (bn > bi + 1) ok[p] = 0;
      if (bn == bi + 1 && i == o0)
        for (int c = 0; c < 3; ++c)
          if (paths.vox[3 * i + c] < cor.boxes[6 * bn + c] || paths.vox[3 * i + c] > cor.boxes[6 * bn + 3 + c]) ok[p] = 0;
    }
    if (ok[p])
      for (int64_t i = o0; i + 1 < o1; ++i) {
        const int64_t bi = box[(size_t)(i - o0)], bn = box[(size_t)(i + 1 - o0)];
        if (bn != bi + 1) continue;
        for (int c = 0; c < 3; ++c) {
          bounds[6 * i + c] = std::max(bounds[6 * i + c], cor.pos[6 * bn + c]);
          bounds[6 * i + 3 + c] = std::min(bounds[6 * i + 3 + c], cor.pos[6 * bn + 3 + c]);
        }
      }
  }
  for (size_t i = 0; i < bounds.size(); ++i)
    if (i % 6 >= 3) bounds[i] -= 0.2 * 0x1p-20;

  fiesta::ESDFMap::RefineParams par;
  par.margin = 0.8, par.w_obstacle = 1.0, par.w_smooth = 2.0, par.alpha = 0.02, par.max_step = 0.05, par.tolerance = 0.0, par.iterations = 32;
  const auto ref = m.RefinePaths(paths.pos, paths.offsets, bounds, par);

  long long n_ok = 0, n_valid = 0, iterations = 0, below = 0, moved = 0;
  double before = 0.0, after = 0.0, far = 0.0;
  size_t longest = 0;
  for (size_t p = 0; p < n; ++p) {
    n_ok += ok[p];
    if (paths.offsets[p + 1] - paths.offsets[p] > paths.offsets[longest + 1] - paths.offsets[longest]) longest = p;
    if (ref.status[p] != FIESTA_HIP_REFINE_OK) continue;
    ++n_valid, iterations += ref.iterations[p], below += ref.n_below[p];
    before += ref.cost[2 * p], after += ref.cost[2 * p + 1];
  }
  for (size_t i = 0; i < ref.pos.size(); ++i) {
    const double d = std::fabs(ref.pos[i] - paths.pos[i]);
    moved += d > 0.0;
    far = std::max(far, d);
  }
  std::printf("%zu paths, %lld inside a whole corridor, %lld refined; J %.6g -> %.6g; the largest move of a coordinate %.3f m\n", n, n_ok, n_valid,
              before, after, far);
  std::printf("the path to (%d, %d, %d), before -> after:\n", frontier[longest](0), frontier[longest](1), frontier[longest](2));
  for (int64_t i = paths.offsets[longest]; i < paths.offsets[longest + 1]; ++i)
    std::printf("  %.3f %.3f %.3f -> %.3f %.3f %.3f\n", paths.pos[3 * i], paths.pos[3 * i + 1], paths.pos[3 * i + 2], ref.pos[3 * i], ref.pos[3 * i + 1],
                ref.pos[3 * i + 2]);
  std::printf("{\"paths\": %zu, \"waypoints\": %zu, \"ok\": %lld, \"valid\": %lld, \"iterations\": %lld, \"n_below\": %lld, \"moved\": %lld, "
              "\"cost_before\": %.17g, \"cost_after\": %.17g, \"largest_move\": %.17g, \"longest\": [%d, %d, %d], \"longest_pos\": [",
              n, paths.pos.size() / 3, n_ok, n_valid, iterations, below, moved, before, after, far, frontier[longest](0), frontier[longest](1),
              frontier[longest](2));
  for (int64_t i = 3 * paths.offsets[longest]; i < 3 * paths.offsets[longest + 1]; ++i)
    std::printf("%s%.17g", i > 3 * paths.offsets[longest] ? ", " : "", ref.pos[i]);
  std::printf("], \"longest_min_dist\": %.17g}\n", ref.min_dist[longest]);
  return 0;
}
