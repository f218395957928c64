// examples/reach_path.cpp -- "and how do I get there?": the last step of the exploration chain through the drop-in class
// (include/fiesta/ESDFMap.h), on the scene of examples/reach.cpp -- 40 x 40 x 20 voxels (0.2 m) seen through one view cone from voxel
// (5, 20, 10) along +x that ends on a wall at x = 30 and holds one pillar, and a pocket behind the wall that is out of reach.
//   GetFrontierVoxels   where known free space ends
//   ReachField          the travel cost from the robot's voxel to every one of them; the map retains the cost field
//   ReachPaths          the path down that field to the cheapest frontier voxel: the raw staircase, and pulled tight by line of sight
//   GetPathCost         the obstacle cost of the tight path, as a trajectory optimiser would start from it
// Prints the path and one JSON line at the end; tests/test_gpu_reach_paths.py builds the same scene through the Python class and
// asserts that the numbers agree.
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
  const int rx = sx + 7;  // the robot has moved into the cone, in front of the pillar
  const std::vector<Eigen::Vector3i> robot{Eigen::Vector3i(rx, sy, sz)};
  std::vector<int32_t> cost;
  m.ReachField(nullptr, nullptr, robot, frontier, 0.0, 26, 0, &cost);

  // the cheapest frontier voxel BEHIND the pillar's plane (the way there bends); among equals the smallest (x, y, z): the frontier
  // call's order is unspecified
  size_t best = 0;
  bool have = false;
  for (size_t i = 0; i < frontier.size(); ++i) {
    if (cost[i] < 0 || cost[i] == INT32_MAX || frontier[i](0) <= 24) continue;
    const auto &a = frontier[i], &b = frontier[best];
    const bool before = a(0) != b(0) ? a(0) < b(0) : (a(1) != b(1) ? a(1) < b(1) : a(2) < b(2));
    if (!have || cost[i] < cost[best] || (cost[i] == cost[best] && before)) best = i, have = true;
  }
  if (!have) {
    std::printf("no frontier voxel behind the pillar can be reached\n");
    return 1;
  }
  const std::vector<Eigen::Vector3i> goal{frontier[best], Eigen::Vector3i(34, 19, 9)};  // ... and a voxel of the pocket
  const auto raw = m.ReachPaths(goal);                  // the field the flood left in the map
  const auto tight = m.ReachPaths(goal, 26, true, 64);  // line-of-sight segments of at most 64 moves
  if (raw.status[0] != FIESTA_HIP_REACH_PATH_OK || tight.status[0] != FIESTA_HIP_REACH_PATH_OK) {
    std::printf("no path: status %d\n", raw.status[0]);
    return 1;
  }
  const std::vector<Eigen::Vector3d> path = tight.Path(0);
  const double pc = m.GetPathCost(path, 0.1, 0.6);
  std::printf("goal (%d, %d, %d) at cost %d: %d moves, %lld raw waypoints, %zu after shortcutting\n", goal[0](0), goal[0](1), goal[0](2),
              cost[best], raw.n_moves[0], (long long)(raw.offsets[1] - raw.offsets[0]), path.size());
  for (size_t i = 0; i < path.size(); ++i)
    std::printf("  (%d, %d, %d)  %.1f %.1f %.1f m\n", tight.vox[3 * i], tight.vox[3 * i + 1], tight.vox[3 * i + 2], path[i](0), path[i](1), path[i](2));
  std::printf("  path cost (step 0.1 m, margin 0.6 m): %.6f\n", pc);
  std::printf("  the pocket voxel: status %d (%s)\n", raw.status[1], raw.status[1] == FIESTA_HIP_REACH_PATH_UNREACHED ? "out of reach" : "?");
  std::printf("{\"goal\": [%d, %d, %d], \"goal_cost\": %d, \"n_moves\": %d, \"raw_waypoints\": %lld, \"waypoints\": [", goal[0](0), goal[0](1),
              goal[0](2), cost[best], raw.n_moves[0], (long long)(raw.offsets[1] - raw.offsets[0]));
  for (size_t i = 0; i < path.size(); ++i)
    std::printf("%s[%d, %d, %d]", i ? ", " : "", tight.vox[3 * i], tight.vox[3 * i + 1], tight.vox[3 * i + 2]);
  std::printf("], \"path_cost\": %.17g, \"pocket_status\": %d, \"pocket_waypoints\": %lld}\n", pc, raw.status[1],
              (long long)(raw.offsets[2] - raw.offsets[1]));
  return 0;
}
