// examples/body_sweep.cpp -- "can the robot make this move?" through the drop-in class (include/fiesta/ESDFMap.h): the doorway scene of
// examples/body_check.cpp -- two rooms, two walls in the plane x = 20 voxels that leave a doorway four voxels (0.8 m) wide -- and its
// robot, a bar of 0.9 m x 0.3 m x 0.2 m modelled as 7 spheres of radius 0.15 m along its long axis.  Three motions from one room into
// the other, each a polyline of poses:
//   lengthwise       the bar points along its path all the way
//   turn in rooms    it starts and ends crosswise, and turns lengthwise before the doorway and back behind it
//   turn in doorway  it starts and ends lengthwise, and is crosswise half way: in the doorway
// BodySweepBatch samples the poses between the waypoints on the device (no centre of a sphere moves farther than `step` between two
// samples), evaluates each as BodyQueryBatch does and returns per motion the tightest sample -- clearance, sphere, pose -- and the
// first sample with a sphere closer than `margin`; IsMotionFree is the scalar convenience.  The first two motions are free, the third
// is not -- although the bar's CENTRE keeps the margin on all three, as PathClearanceBatch on the same positions reports.  Prints one
// line per motion and one JSON line at the end, with the poses it used (a test that repeats the motions elsewhere need not repeat the
// sine and cosine); tests/test_cpp_body_sweep.py builds the same scene through the Python class and asserts that the numbers agree.
#include <array>
#include <cmath>
#include <cstdio>
#include <vector>

#include "fiesta/ESDFMap.h"

int main() {
  fiesta::ESDFMap m(Eigen::Vector3d(-4.0, -4.0, 0.0), 0.2, Eigen::Vector3d(8.0, 8.0, 4.0));  // 40 x 40 x 20 voxels
  m.SetParameters(0.70, 0.35, 0.12, 0.97, 0.80);
  m.SetOriginalRange();
  const int wall = 20, post_lo = 17, post_hi = 22;  // the walls: x = 20, y <= 17 and y >= 22; the doorway: y = 18 .. 21
  for (int cycle = 0; cycle < 3; ++cycle) {          // (an obstacle needs three hits to count as occupied)
    for (int x = 0; x < 40; ++x)
      for (int y = 0; y < 40; ++y)
        for (int z = 0; z < 20; ++z) {
          const bool hit = x == wall && (y <= post_lo || y >= post_hi);
          if (cycle == 0 || hit) m.SetOccupancy(Eigen::Vector3i(x, y, z), hit ? 1 : 0);
        }
    m.UpdateOccupancy(true);
  }
  m.UpdateESDF();

  fiesta::ESDFMap::BodySpheres bar;
  for (int i = -3; i <= 3; ++i) bar.push_back({0.1 * i, 0.0, 0.0, 0.15});  // centres every 0.1 m, the tips at +-0.45 m
  const double step = 0.05, margin = 0.1, half = 0.5 * 1.57079632679489661923;
  const std::array<double, 4> along = {1.0, 0.0, 0.0, 0.0}, across = {std::cos(half), 0.0, 0.0, std::sin(half)};  // yaw 0 and 90 degrees
  const auto pose = [](double x, const std::array<double, 4> &q) { return std::array<double, 7>{x, 0.0, 2.0, q[0], q[1], q[2], q[3]}; };
  const char *names[3] = {"lengthwise", "turn in rooms", "turn in doorway"};
  const fiesta::ESDFMap::BodyPoses motions[3] = {{pose(-1.5, along), pose(1.7, along)},
                                                 {pose(-1.5, across), pose(-0.7, along), pose(0.9, along), pose(1.7, across)},
                                                 {pose(-1.5, along), pose(0.1, across), pose(1.7, along)}};
  fiesta::ESDFMap::BodyPoses all;
  std::vector<int64_t> offsets = {0};
  std::vector<double> centres;
  for (const auto &mo : motions) {
    for (const auto &p : mo) all.push_back(p), centres.insert(centres.end(), {p[0], p[1], p[2]});
    offsets.push_back((int64_t)all.size());
  }
  const fiesta::ESDFMap::SweepResult r = m.BodySweepBatch(bar, all, offsets, step, margin);
  double centre_min[3];
  int64_t centre_first[3];
  m.PathClearanceBatch(centres.data(), (int64_t)all.size(), offsets.data(), 3, step, margin,
                       fiesta_hip_path_result{centre_min, nullptr, nullptr, nullptr, centre_first, nullptr, nullptr});
  for (int k = 0; k < 3; ++k) {
    const bool free_scalar = m.IsMotionFree(bar, motions[k], step, margin);
    std::printf("%-15s: %s  %lld samples, tightest %.3f m at sample %lld (x = %.2f m), sphere %d", names[k], free_scalar ? "free   " : "blocked",
                (long long)r.n_samples[k], r.min_clearance[k], (long long)r.min_sample[k], r.min_pose[k][0], r.min_sphere[k]);
    if (r.first_below[k] >= 0)
      std::printf("; first contact at sample %lld (x = %.2f m), sphere %d, %lld samples in contact", (long long)r.first_below[k],
                  r.first_below_pose[k][0], r.first_below_sphere[k], (long long)r.n_below[k]);
    std::printf("; the centre alone keeps %.3f m\n", centre_min[k]);
    if (free_scalar != (r.first_below[k] < 0) || centre_first[k] >= 0) return 1;
  }

  std::printf("{\"step\": %.17g, \"margin\": %.17g, \"spheres\": [", step, margin);
  for (size_t i = 0; i < bar.size(); ++i) std::printf("%s[%.17g, %.17g, %.17g, %.17g]", i ? ", " : "", bar[i][0], bar[i][1], bar[i][2], bar[i][3]);
  std::printf("], \"motions\": [");
  for (int k = 0; k < 3; ++k) {
    std::printf("%s{\"name\": \"%s\", \"poses\": [", k ? ", " : "", names[k]);
    for (size_t i = 0; i < motions[k].size(); ++i) {
      const auto &p = motions[k][i];
      std::printf("%s[%.17g, %.17g, %.17g, %.17g, %.17g, %.17g, %.17g]", i ? ", " : "", p[0], p[1], p[2], p[3], p[4], p[5], p[6]);
    }
    std::printf("], \"free\": %s, \"n_samples\": %lld, \"min_clearance\": %.17g, \"min_sample\": %lld, \"min_sphere\": %d, \"first_below\": %lld, "
                "\"first_below_sphere\": %d, \"n_below\": %lld, \"centre_min_dist\": %.17g}",
                r.first_below[k] < 0 ? "true" : "false", (long long)r.n_samples[k], r.min_clearance[k], (long long)r.min_sample[k], r.min_sphere[k],
                (long long)r.first_below[k], r.first_below_sphere[k], (long long)r.n_below[k], centre_min[k]);
  }
  std::printf("]}\n");
  return 0;
}
