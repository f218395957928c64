// examples/corridor_bounds.cpp -- the planner chain's last two links through the drop-in class (include/fiesta/ESDFMap.h), on the
// scene of examples/corridor.cpp -- 40 x 40 x 20 voxels (0.2 m) seen through one view cone from voxel (5, 20, 10) along +x that ends
// on a wall at x = 30 and holds one pillar.
//   GetFrontierVoxels, ReachField   where known free space ends, and the travel cost from the robot's voxel to all of it
//   ReachPaths                      the RAW paths to every frontier voxel: voxel staircases, one waypoint per move
//   PathCorridor                    per path the safe flight corridor, here inside a window that ends at z = 13: the paths that climb
//                                   above it are BLOCKED there, their corridors are not whole
//   CorridorBounds                  per waypoint the box it may move in, on the device (examples/path_refine.cpp does this step by
//                                   hand); VOID_BROKEN: the paths without a whole corridor get NaN rows
//   RefinePaths                     every path with a whole corridor descends inside its boxes; the others come back INVALID, unmoved
// Prints one JSON line at the end; tests/test_cpp_bounds.py builds the same scene through the Python class and asserts that the
// numbers agree.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
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
  const Eigen::Vector3i lo(0, 0, 0), hi(39, 39, 13);
  const auto cor = m.PathCorridor(paths.vox, paths.offsets, 8, 0.0, 0, &lo, &hi);
  const auto bnd = m.CorridorBounds(paths.vox, paths.offsets, cor, -1, true);

  fiesta::ESDFMap::RefineParams par;
  par.margin = 0.8, par.w_obstacle = 1.0, par.w_smooth = 2.0, par.alpha = 0.02, par.max_step = 0.05, par.tolerance = 0.0, par.iterations = 32;
  const auto ref = m.RefinePaths(paths.pos, paths.offsets, bnd.bounds, par);

  const size_t n = frontier.size(), nw = paths.pos.size() / 3;
  long long n_ok = 0, n_valid = 0, nan_rows = 0, boxed = 0, moved = 0;
  uint64_t checksum = 0;  // the sum of the bounds' bit patterns, modulo 2^64
  size_t longest = 0;
  for (size_t p = 0; p < n; ++p) {
    n_ok += bnd.ok[p] != 0, n_valid += ref.status[p] == FIESTA_HIP_REFINE_OK;
    if (paths.offsets[p + 1] - paths.offsets[p] > paths.offsets[longest + 1] - paths.offsets[longest]) longest = p;
  }
  for (size_t i = 0; i < nw; ++i) {
    nan_rows += std::isnan(bnd.bounds[6 * i]);
    boxed += bnd.box[i] >= 0;
    for (int c = 0; c < 6; ++c) {
      uint64_t u;
      std::memcpy(&u, &bnd.bounds[6 * i + c], 8);
      checksum += u;
    }
    for (int c = 0; c < 3; ++c) moved += ref.pos[3 * i + c] != paths.pos[3 * i + c];
  }
  std::printf("%zu paths, %zu waypoints, %zu boxes; %lld corridors whole, %lld rows void, %lld paths refined, %lld coordinates moved\n", n, nw,
              cor.entry.size(), n_ok, nan_rows, n_valid, moved);
  std::printf("{\"paths\": %zu, \"waypoints\": %zu, \"boxes\": %zu, \"ok\": %lld, \"nan_rows\": %lld, \"boxed\": %lld, \"checksum\": %llu, \"valid\": %lld, "
              "\"moved\": %lld, \"longest\": [%d, %d, %d], \"longest_ok\": %d, \"longest_pos\": [",
              n, nw, cor.entry.size(), n_ok, nan_rows, boxed, (unsigned long long)checksum, n_valid, moved, frontier[longest](0), frontier[longest](1),
              frontier[longest](2), (int)bnd.ok[longest]);
  for (int64_t i = 3 * paths.offsets[longest]; i < 3 * paths.offsets[longest + 1]; ++i)
    std::printf("%s%.17g", i > 3 * paths.offsets[longest] ? ", " : "", ref.pos[i]);
  std::printf("]}\n");
  return 0;
}
