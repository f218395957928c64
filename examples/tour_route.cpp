// examples/tour_route.cpp -- "in which order, and along which way?" through the drop-in class (include/fiesta/ESDFMap.h): the scene
// and the sites of examples/frontier_tour.cpp -- a room seen through one view cone that ends on a wall and holds a pillar, the robot
// and the best pose of every frontier piece.
//   TourRoute   ReachMatrix (one flood per site, side by side) -> SiteTour (the order) -> LegPaths (the way along every leg, read out
//               of the floods the matrix call left on the device: nothing is flooded twice), pulled tight by line of sight
//   PathCorridor  the legs go on as they are -- CSR offsets over voxel waypoints -- into the safe flight corridors
// The frontier call's order is unspecified and cluster ids follow it, so the pose voxels are sorted (and listed once) before they
// become sites: the output is the same on every run.  Prints the route and one JSON line at the end; tests/test_cpp_leg_paths.py
// builds the same scene through the Python class and asserts that the numbers agree.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <vector>

#include "fiesta/ESDFMap.h"

template <typename T>
static void print_list(const char *name, const std::vector<T> &v, const char *tail) {
  std::printf("\"%s\": [", name);
  for (size_t k = 0; k < v.size(); ++k) std::printf("%s%lld", k ? ", " : "", (long long)v[k]);
  std::printf("]%s", tail);
}

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
  std::vector<std::array<int, 3>> pose;  // the voxel of every cluster's best pose, once per box of a 3 x 2 grid over y and z
  const int ycut[4] = {0, 14, 27, 40}, zcut[3] = {0, 10, 20};
  for (int by = 0; by < 3; ++by)
    for (int bz = 0; bz < 2; ++bz) {
      const Eigen::Vector3i lo(0, ycut[by], zcut[bz]), hi(39, ycut[by + 1] - 1, zcut[bz + 1] - 1);
      std::vector<Eigen::Vector3i> frontier;
      const fiesta::ESDFMap::FrontierViewSet f = m.GetFrontierViews(&lo, &hi, 0.0, 26, 5, ring, cam, frontier);
      for (size_t k = 0; k < f.best_pos.size(); ++k) {
        if (f.coverage.best_view[k] < 0) continue;
        std::array<int, 3> v;
        for (int c = 0; c < 3; ++c) v[(size_t)c] = (int)std::floor((f.best_pos[k](c) - org[c]) / res);
        pose.push_back(v);
      }
    }
  std::sort(pose.begin(), pose.end());
  pose.erase(std::unique(pose.begin(), pose.end()), pose.end());
  std::vector<Eigen::Vector3i> sites{Eigen::Vector3i(sx + 7, sy, sz)};  // the robot has moved into the cone
  for (const auto &v : pose) sites.push_back(Eigen::Vector3i(v[0], v[1], v[2]));

  const fiesta::ESDFMap::TourRouteResult r = m.TourRoute(sites, 0, false, nullptr, nullptr, 0.0, 26, 0, 64, 2024, 0, true, 64);
  const fiesta::ESDFMap::ReachPathSet &p = r.legs.paths;
  std::printf("%zu sites, %d within reach, tour length %lld = %.2f m\n", sites.size(), r.tour.info.n_visited, (long long)r.tour.info.length,
              r.tour.info.length * res / 3.0);
  for (size_t k = 0; k < r.leg_from.size(); ++k)
    std::printf("  leg %2zu: site %2d -> %2d, cost %4d, %3d moves, %2lld waypoints\n", k, r.leg_from[k], r.leg_to[k], r.legs.cost[k], p.n_moves[k],
                (long long)(p.offsets[k + 1] - p.offsets[k]));
  // the legs as they are, on into the corridors
  const fiesta::ESDFMap::CorridorSet c = m.PathCorridor(p.vox, p.offsets, 8);
  std::printf("%zu waypoints in %zu legs, %lld corridor boxes\n", p.vox.size() / 3, r.leg_from.size(), (long long)c.offsets.back());

  std::printf("{\"sites\": [");
  for (size_t i = 0; i < sites.size(); ++i) std::printf("%s[%d, %d, %d]", i ? ", " : "", sites[i](0), sites[i](1), sites[i](2));
  std::printf("], ");
  print_list("order", r.tour.order, ", ");
  print_list("tour_leg_cost", r.tour.leg_cost, ", ");
  print_list("from", r.leg_from, ", ");
  print_list("to", r.leg_to, ", ");
  print_list("offsets", p.offsets, ", ");
  print_list("status", p.status, ", ");
  print_list("n_moves", p.n_moves, ", ");
  print_list("cost", r.legs.cost, ", ");
  print_list("waypoints_vox", p.vox, ", ");
  print_list("corridor_offsets", c.offsets, ", ");
  std::printf("\"waypoints_pos\": [");
  for (size_t k = 0; k < p.pos.size(); ++k) std::printf("%s%.17g", k ? ", " : "", p.pos[k]);
  std::printf("], \"length\": %lld, \"n_sources\": %lld, \"connectivity\": %d}\n", (long long)r.tour.info.length, (long long)r.legs.info.n_sources,
              r.legs.info.connectivity);
  bool ok = !r.leg_from.empty();
  for (size_t k = 0; k < r.leg_from.size(); ++k) ok = ok && p.status[k] == FIESTA_HIP_REACH_PATH_OK && r.legs.cost[k] == r.tour.leg_cost[k + 1];
  return ok ? 0 : 1;
}
