// examples/frontier_clusters.cpp -- "which frontier next?" through the drop-in class (include/fiesta/ESDFMap.h): the scene of
// examples/reach.cpp -- a room seen through one view cone that ends on a wall and holds a pillar, and a pocket of free space behind
// the wall that touches the cone nowhere.
//   GetFrontierVoxels   where known free space ends: single voxels
//   ReachField          the travel cost from the robot's voxel to every one of them
//   ClusterVoxels       the FRONTIERS: connected groups of those voxels, specks below min_size dropped, each with its size, box and
//                       centroid (where to place a viewpoint) and -- with key = the travel costs -- its cheapest reachable member
//   ReachPaths          the paths to those cheapest members, out of the field the flood left in the map
// The frontier call's order is unspecified and cluster ids follow the list's order, so the list is sorted first: the output is the
// same on every run.  Prints the clusters and one JSON line at the end; tests/test_cpp_clusters.py builds the same scene through the
// Python class and asserts that the numbers agree.
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

  std::vector<Eigen::Vector3i> found, frontier;
  std::vector<uint8_t> found_mask, mask;
  m.GetFrontierVoxels(0.0, found, &found_mask);
  std::vector<size_t> order(found.size());
  std::iota(order.begin(), order.end(), (size_t)0);
  std::sort(order.begin(), order.end(), [&](size_t i, size_t j) {
    const auto &a = found[i], &b = found[j];
    return a(0) != b(0) ? a(0) < b(0) : (a(1) != b(1) ? a(1) < b(1) : a(2) < b(2));
  });
  for (size_t i : order) frontier.push_back(found[i]), mask.push_back(found_mask[i]);

  const int rx = sx + 7;  // the robot has moved into the cone
  const std::vector<Eigen::Vector3i> robot{Eigen::Vector3i(rx, sy, sz)};
  std::vector<int32_t> cost;
  m.ReachField(nullptr, nullptr, robot, frontier, 0.0, 26, 0, &cost);  // (its field stays in the map: ReachPaths below descends it)

  const int32_t min_size = 5;
  const fiesta::ESDFMap::VoxelClusters c = m.ClusterVoxels(frontier, &mask, &cost, 26, min_size);
  std::printf("frontier voxels: %zu in %lld clusters of at least %d (%lld smaller ones dropped), largest %lld\n", frontier.size(),
              (long long)c.info.n_clusters, min_size, (long long)c.info.n_dropped_clusters, (long long)c.info.largest);
  std::vector<Eigen::Vector3i> goals;
  for (size_t k = 0; k < c.count(); ++k) {
    std::printf("  cluster %zu: %d voxels, box (%d, %d, %d) .. (%d, %d, %d), centroid (%.3f, %.3f, %.3f) m, unknown sides 0x%02x", k, c.size[k],
                c.box_lo[k](0), c.box_lo[k](1), c.box_lo[k](2), c.box_hi[k](0), c.box_hi[k](1), c.box_hi[k](2), c.centroid[k](0), c.centroid[k](1),
                c.centroid[k](2), c.mask_or[k]);
    if (c.key_argmin[k] >= 0 && c.key_min[k] != INT32_MAX) {
      const auto &v = frontier[(size_t)c.key_argmin[k]];
      std::printf(", cheapest member (%d, %d, %d) at cost %d = %.2f m\n", v(0), v(1), v(2), c.key_min[k], c.key_min[k] * 0.2 / 3.0);
      goals.push_back(v);
    } else {
      std::printf(", out of reach\n");
    }
  }
  const fiesta::ESDFMap::ReachPathSet paths = m.ReachPaths(goals, 26, true);
  for (size_t p = 0; p < goals.size(); ++p)
    std::printf("  path to (%d, %d, %d): %d moves, %lld waypoints after shortcutting\n", goals[p](0), goals[p](1), goals[p](2), paths.n_moves[p],
                (long long)(paths.offsets[p + 1] - paths.offsets[p]));

  std::printf("{\"frontier\": %zu, \"n_clusters\": %lld, \"n_dropped_clusters\": %lld, \"n_members\": %lld, \"largest\": %lld, \"clusters\": [",
              frontier.size(), (long long)c.info.n_clusters, (long long)c.info.n_dropped_clusters, (long long)c.info.n_members,
              (long long)c.info.largest);
  for (size_t k = 0; k < c.count(); ++k)
    std::printf("%s{\"size\": %d, \"root\": %lld, \"box_lo\": [%d, %d, %d], \"box_hi\": [%d, %d, %d], \"centroid\": [%.17g, %.17g, %.17g], "
                "\"mask_or\": %d, \"key_min\": %d, \"key_argmin\": %lld}",
                k ? ", " : "", c.size[k], (long long)c.root[k], c.box_lo[k](0), c.box_lo[k](1), c.box_lo[k](2), c.box_hi[k](0), c.box_hi[k](1),
                c.box_hi[k](2), c.centroid[k](0), c.centroid[k](1), c.centroid[k](2), (int)c.mask_or[k], c.key_min[k], (long long)c.key_argmin[k]);
  std::printf("], \"path_moves\": [");
  for (size_t p = 0; p < goals.size(); ++p) std::printf("%s%d", p ? ", " : "", paths.n_moves[p]);
  std::printf("], \"path_waypoints\": %lld}\n", (long long)paths.offsets[goals.size()]);
  return 0;
}
