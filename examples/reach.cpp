// examples/reach.cpp -- the exploration loop's "where to next?" through the drop-in class (include/fiesta/ESDFMap.h):
// the room of examples/frontiers.cpp -- 40 x 40 x 20 voxels (0.2 m) seen through ONE view cone from voxel (5, 20, 10) along +x that
// ends on a wall at x = 30 and holds one pillar -- and a second pocket of free space, seen once through a window, that touches the
// cone nowhere.
//   GetFrontierVoxels   where known free space ends
//   ReachField          the travel cost from the robot's voxel to every one of them (they are the call's targets): the pocket's
//                       frontier voxels are free and have clearance, and are out of reach all the same
// Prints the counts, the nearest reachable frontier voxel and one JSON line at the end; tests/test_cpp_reach.py builds the same
// scene through the Python class and asserts that the numbers agree.
#include <climits>
#include <cstdio>
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
  const int rx = sx + 7;  // the robot has moved into the cone
  const std::vector<Eigen::Vector3i> robot{Eigen::Vector3i(rx, sy, sz)};
  std::vector<int32_t> cost, cost_clear;
  const fiesta_hip_reach_info info = m.ReachField(nullptr, nullptr, robot, frontier, 0.0, 26, 0, &cost);
  m.ReachField(nullptr, nullptr, robot, frontier, 0.3, 26, 0, &cost_clear);  // ... for a robot of 0.3 m radius

  size_t reachable = 0, reachable_clear = 0, out_of_reach = 0, best = 0;
  long long sum = 0;
  bool have = false;
  for (size_t i = 0; i < frontier.size(); ++i) {
    if (cost[i] == INT32_MAX) ++out_of_reach;
    if (cost_clear[i] >= 0 && cost_clear[i] != INT32_MAX) ++reachable_clear;
    if (cost[i] < 0 || cost[i] == INT32_MAX) continue;
    ++reachable;
    sum += cost[i];
    // the nearest one; among equals the smallest (x, y, z): the frontier call's order is unspecified
    const auto &a = frontier[i], &b = frontier[best];
    const bool before = a(0) != b(0) ? a(0) < b(0) : (a(1) != b(1) ? a(1) < b(1) : a(2) < b(2));
    if (!have || cost[i] < cost[best] || (cost[i] == cost[best] && before)) best = i, have = true;
  }
  if (!have) {
    std::printf("no frontier voxel can be reached\n");
    return 1;
  }
  std::printf("frontier voxels: %zu, reachable from (%d, %d, %d): %zu, out of reach: %zu\n", frontier.size(), rx, sy, sz, reachable, out_of_reach);
  std::printf("  reachable with 0.3 m clearance: %zu\n", reachable_clear);
  std::printf("  nearest: (%d, %d, %d) at cost %d = %.2f m\n", frontier[best](0), frontier[best](1), frontier[best](2), cost[best],
              cost[best] * 0.2 / 3.0);
  std::printf("  flood: %lld of %lld traversable voxels reached in %lld rounds\n", (long long)info.n_reached, (long long)info.n_traversable,
              (long long)info.rounds);
  std::printf("{\"frontier\": %zu, \"reachable\": %zu, \"out_of_reach\": %zu, \"reachable_clear\": %zu, \"nearest\": [%d, %d, %d], "
              "\"nearest_cost\": %d, \"cost_sum\": %lld, \"n_reached\": %lld, \"n_traversable\": %lld, \"max_cost\": %lld}\n",
              frontier.size(), reachable, out_of_reach, reachable_clear, frontier[best](0), frontier[best](1), frontier[best](2), cost[best], sum,
              (long long)info.n_reached, (long long)info.n_traversable, (long long)info.max_cost);
  return 0;
}
