// examples/reach_matrix.cpp -- "in which order?" through the drop-in class (include/fiesta/ESDFMap.h): the scene of
// examples/reach.cpp -- a room seen through one view cone that ends on a wall and holds a pillar, and a pocket of free space behind
// the wall that touches the cone nowhere.
//   GetFrontierVoxels   where known free space ends
//   ReachField          the travel cost from the robot's voxel to every one of them
//   ClusterVoxels       the frontiers, each with its cheapest member by that cost (key_argmin): the SITES, with the robot as site 0
//   ReachMatrix         the travel cost between every pair of sites, the floods of all sites side by side: the matrix a tour
//                       solver takes.  The pocket's site is free and out of reach: INT32_MAX along its row and column, 0 on the diagonal
// ... and the simplest solver: a greedy nearest-neighbour tour from the robot over the sites it can reach (ties: the lower index).
// The frontier call's order is unspecified and cluster ids follow the list's order, so the list is sorted first: the output is the
// same on every run.  Prints the matrix and one JSON line at the end; tests/test_cpp_reach_matrix.py builds the same scene through
// the Python class and asserts that the numbers agree.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <numeric>
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
  const std::vector<Eigen::Vector3i> robot{Eigen::Vector3i(sx + 7, sy, sz)};  // the robot has moved into the cone
  std::vector<int32_t> key;
  m.ReachField(nullptr, nullptr, robot, frontier, 0.0, 26, 0, &key);
  const fiesta::ESDFMap::VoxelClusters c = m.ClusterVoxels(frontier, nullptr, &key, 26, 5);

  std::vector<Eigen::Vector3i> sites = robot;
  for (size_t k = 0; k < c.count(); ++k)
    if (c.key_argmin[k] >= 0) sites.push_back(frontier[(size_t)c.key_argmin[k]]);
  const size_t n = sites.size();
  std::vector<int32_t> cost, status;
  const fiesta_hip_reach_matrix_info info = m.ReachMatrix(nullptr, nullptr, sites, {}, 0.0, 26, 0, &cost, &status);
  std::printf("%zu sites (the robot and %zu frontier clusters): %lld floods side by side in %lld batch(es), %lld rounds, %lld tile visits\n", n,
              n - 1, (long long)info.fields, (long long)info.batches, (long long)info.rounds, (long long)info.tile_visits);
  long long checksum = 0;
  size_t unreached = 0, blocked = 0;
  for (size_t i = 0; i < n; ++i) {
    std::printf("  site %zu (%2d, %2d, %2d) status %d:", i, sites[i](0), sites[i](1), sites[i](2), status[i]);
    for (size_t j = 0; j < n; ++j) {
      const int32_t v = cost[i * n + j];
      if (v == INT32_MAX)
        ++unreached, std::printf("    -");
      else if (v < 0)
        ++blocked, std::printf("    x");
      else
        checksum += v, std::printf(" %4d", v);
    }
    std::printf("\n");
  }

  // greedy nearest neighbour from the robot; among equals the lower site index
  std::vector<size_t> tour{0};
  std::vector<bool> seen(n, false);
  seen[0] = true;
  long long length = 0;
  for (;;) {
    const size_t at = tour.back();
    size_t best = n;
    for (size_t j = 0; j < n; ++j) {
      const int32_t v = cost[at * n + j];
      if (seen[j] || v < 0 || v == INT32_MAX) continue;
      if (best == n || v < cost[at * n + best]) best = j;
    }
    if (best == n) break;
    length += cost[at * n + best];
    seen[best] = true;
    tour.push_back(best);
  }
  std::printf("tour:");
  for (size_t s : tour) std::printf(" %zu", s);
  std::printf(", length %lld = %.2f m; %zu site(s) out of reach\n", length, length * 0.2 / 3.0, n - tour.size());

  std::printf("{\"sites\": %zu, \"checksum\": %lld, \"unreached\": %zu, \"blocked\": %zu, \"tour\": [", n, checksum, unreached, blocked);
  for (size_t i = 0; i < tour.size(); ++i) std::printf("%s%zu", i ? ", " : "", tour[i]);
  std::printf("], \"tour_length\": %lld}\n", length);
  return 0;
}
