// examples/path_timing.cpp -- "which frontier is nearest -- in seconds": the step after the paths, through the drop-in class
// (include/fiesta/ESDFMap.h), on the scene of examples/corridor.cpp -- 40 x 40 x 20 voxels (0.2 m) seen through one view cone from
// voxel (5, 20, 10) along +x that ends on a wall at x = 30 and holds one pillar.
//   GetFrontierVoxels, ReachField   where known free space ends, and the travel cost from the robot's voxel to all of it
//   ReachPaths                      the paths to every frontier voxel, as CSR polylines in metres
//   PathTiming                      per path the travel time under a clearance-limited speed profile: the robot brakes near
//                                   obstacles, slows at bends, starts and ends at rest and accelerates no faster than a_max
// Prints the frontier voxel nearest in metres and the one nearest in seconds, and one JSON line at the end; tests/test_cpp_path_timing.py
// builds the same scene through the Python class and asserts that the numbers agree.
#include <algorithm>
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
  std::sort(frontier.begin(), frontier.end(), [](const Eigen::Vector3i &a, const Eigen::Vector3i &b) {
    return a(0) != b(0) ? a(0) < b(0) : (a(1) != b(1) ? a(1) < b(1) : a(2) < b(2));
  });
  const std::vector<Eigen::Vector3i> robot{Eigen::Vector3i(sx + 7, sy, sz)};
  m.ReachField(nullptr, nullptr, robot, {}, 0.0, 26, 0, nullptr);
  const auto paths = m.ReachPaths(frontier, 26, false);

  fiesta::ESDFMap::TimingParams par;
  par.step = 0.2, par.margin = 0.3, par.v_max = 2.0, par.v_min = 0.1, par.a_max = 1.5, par.corner_dev = 0.05;
  const auto t = m.PathTiming(paths.pos, paths.offsets, par);

  const size_t n = frontier.size();
  long long timed = 0, samples = 0, slowed = 0;
  double total = 0.0;
  long long by_time = -1, by_length = -1;  // among the paths of at least two waypoints: ties to the lowest index
  for (size_t p = 0; p < n; ++p) {
    if (t.status[p] != FIESTA_HIP_TIMING_OK || t.n_samples[p] < 2) continue;
    ++timed, samples += t.n_samples[p], slowed += t.n_below[p] > 0;
    total += t.duration[p];
    if (by_time < 0 || t.duration[p] < t.duration[(size_t)by_time]) by_time = (long long)p;
    if (by_length < 0 || t.length[p] < t.length[(size_t)by_length]) by_length = (long long)p;
  }
  if (by_time < 0) {
    std::printf("no frontier voxel is reachable\n");
    return 1;
  }
  const Eigen::Vector3i ft = frontier[(size_t)by_time], fl = frontier[(size_t)by_length];
  std::printf("%zu frontier voxels, %lld timed paths of %lld samples, %lld of them below the margin somewhere; %.3f s in all\n", n, timed, samples,
              slowed, total);
  std::printf("nearest in metres:  (%d, %d, %d), %.3f m, %.3f s\n", fl(0), fl(1), fl(2), t.length[(size_t)by_length], t.duration[(size_t)by_length]);
  std::printf("nearest in seconds: (%d, %d, %d), %.3f m, %.3f s\n", ft(0), ft(1), ft(2), t.length[(size_t)by_time], t.duration[(size_t)by_time]);
  std::printf("{\"paths\": %zu, \"timed\": %lld, \"samples\": %lld, \"duration\": %.17g, \"below\": %lld, \"nearest_time\": [%d, %d, %d], "
              "\"nearest_time_duration\": %.17g, \"nearest_length\": [%d, %d, %d], \"nearest_length_length\": %.17g}\n",
              n, timed, samples, total, slowed, ft(0), ft(1), ft(2), t.duration[(size_t)by_time], fl(0), fl(1), fl(2), t.length[(size_t)by_length]);
  return 0;
}
