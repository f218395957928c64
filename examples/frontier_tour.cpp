// examples/frontier_tour.cpp -- "where next, and in which order after that?" through the drop-in class (include/fiesta/ESDFMap.h):
// the scene of examples/frontier_views.cpp -- a room seen through one view cone that ends on a wall and holds a pillar, and a pocket
// of free space behind the wall.
//   GetFrontierViews   the frontiers and, for each, the pose of a ring around its centroid that sees most of it -- once per box of
//                      a 3 x 2 grid over y and z, which cuts the one large frontier of this scene into pieces worth a visit each
//   ReachMatrix        the travel cost between every pair of sites: the robot (site 0) and the voxel of every best pose
//   SiteTour           the order in which to visit the sites the robot can reach: 64 local searches side by side, open path
// The frontier call's order is unspecified and cluster ids follow it, so the pose voxels are sorted (and listed once) before they
// become sites: the output is the same on every run.  Prints the tour and one JSON line at the end; tests/test_cpp_tour.py builds
// the same scene through the Python class and asserts that the numbers agree.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <vector>

#include "fiesta/ESDFMap.h"

int main() {
  const double org[3] = {-4.0, -4.0, 0.0}, res = 0.2;
  fiesta::ESDFMap m(Eigen::Vector3d(org[0], org[1], org[2]), res, Eigen::Vector3d(8.0, 8.0, 4.0));  // 40 x 40 x 20 voxels
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

  const std::vector<fiesta::ESDFMap::RingRow> ring = fiesta::ESDFMap::ViewRing({0.8, 1.6}, 12, {0.0});
  const double deg = 3.141592653589793 / 180.0;
  const fiesta_hip_view_sensor cam = fiesta::ESDFMap::ViewSensor(0.2, 3.0, std::tan(40.0 * deg), std::tan(30.0 * deg),
                                                                 FIESTA_HIP_RAY_OCCUPIED | FIESTA_HIP_RAY_UNKNOWN, false, 0.3, 3);
  // like a planner that splits large frontiers before it places viewpoints: the chain once per box of a 3 x 2 grid over y and z
  std::vector<std::array<int, 3>> pose;  // the voxel of every cluster's best pose
  const int ycut[4] = {0, 14, 27, 40}, zcut[3] = {0, 10, 20};
  for (int by = 0; by < 3; ++by)
    for (int bz = 0; bz < 2; ++bz) {
      const Eigen::Vector3i lo(0, ycut[by], zcut[bz]), hi(39, ycut[by + 1] - 1, zcut[bz + 1] - 1);
      std::vector<Eigen::Vector3i> frontier;
      const fiesta::ESDFMap::FrontierViewSet f = m.GetFrontierViews(&lo, &hi, 0.0, 26, 5, ring, cam, frontier);
      size_t posed = 0;
      for (size_t k = 0; k < f.best_pos.size(); ++k) {
        if (f.coverage.best_view[k] < 0) continue;
        std::array<int, 3> v;
        for (int c = 0; c < 3; ++c) v[(size_t)c] = (int)std::floor((f.best_pos[k](c) - org[c]) / res);
        pose.push_back(v), ++posed;
      }
      std::printf("box y %2d..%2d z %2d..%2d: %zu frontier voxels in %zu clusters, %zu with a pose\n", lo(1), hi(1), lo(2), hi(2), frontier.size(),
                  f.clusters.count(), posed);
    }
  std::sort(pose.begin(), pose.end());
  pose.erase(std::unique(pose.begin(), pose.end()), pose.end());
  std::vector<Eigen::Vector3i> sites{Eigen::Vector3i(sx + 7, sy, sz)};  // the robot has moved into the cone
  for (const auto &v : pose) sites.push_back(Eigen::Vector3i(v[0], v[1], v[2]));
  const int32_t n = (int32_t)sites.size();

  std::vector<int32_t> cost;
  m.ReachMatrix(nullptr, nullptr, sites, {}, 0.0, 26, 0, &cost);
  const fiesta::ESDFMap::SiteTourResult t = m.SiteTour(cost, n, 0, false, 64, 2024);
  std::printf("%d sites (the robot and %d poses), %d of them within reach; %d restarts made %lld moves, restart %d is the best\n", n, n - 1,
              t.info.n_visited, 64, (long long)t.info.moves, t.info.best_restart);
  for (size_t k = 0; k < t.order.size(); ++k) {
    const Eigen::Vector3i &v = sites[(size_t)t.order[k]];
    std::printf("  %2zu: site %2d (%2d, %2d, %2d) after %4d\n", k, t.order[k], v(0), v(1), v(2), t.leg_cost[k]);
  }
  std::printf("length %lld = %.2f m; the nearest-neighbour tour: %lld\n", (long long)t.info.length, t.info.length * res / 3.0,
              (long long)t.info.nn_length);

  std::printf("{\"sites\": [");
  for (int32_t i = 0; i < n; ++i) std::printf("%s[%d, %d, %d]", i ? ", " : "", sites[(size_t)i](0), sites[(size_t)i](1), sites[(size_t)i](2));
  std::printf("], \"order\": [");
  for (size_t k = 0; k < t.order.size(); ++k) std::printf("%s%d", k ? ", " : "", t.order[k]);
  std::printf("], \"leg_cost\": [");
  for (size_t k = 0; k < t.leg_cost.size(); ++k) std::printf("%s%d", k ? ", " : "", t.leg_cost[k]);
  std::printf("], \"site_status\": [");
  for (size_t k = 0; k < t.site_status.size(); ++k) std::printf("%s%d", k ? ", " : "", t.site_status[k]);
  std::printf("], \"restart_length\": [");
  for (size_t k = 0; k < t.restart_length.size(); ++k) std::printf("%s%lld", k ? ", " : "", (long long)t.restart_length[k]);
  std::printf("], \"n_visited\": %d, \"length\": %lld, \"nn_length\": %lld, \"best_restart\": %d, \"moves\": %lld, \"capped\": %lld}\n", t.info.n_visited,
              (long long)t.info.length, (long long)t.info.nn_length, t.info.best_restart, (long long)t.info.moves, (long long)t.info.capped);
  return t.info.length <= t.info.nn_length ? 0 : 1;
}
