// examples/body_check.cpp -- "does the robot fit through the door at this heading?" through the drop-in class
// (include/fiesta/ESDFMap.h): the doorway scene of examples/skeleton.cpp -- two rooms, two walls in the plane x = 20 voxels that
// leave a doorway four voxels (0.8 m) wide.  The robot is a bar of 0.9 m x 0.3 m x 0.2 m, modelled as 7 spheres of radius 0.15 m
// along its long axis, and stands in the middle of the doorway at 12 yaw angles, 15 degrees apart.
//   BodyQueryBatch   per pose the clearance of the closest sphere, which sphere that is, and the obstacle penalty with its derivative
//                    with respect to the pose (a force and a torque)
//   IsPoseFree       the scalar convenience: min_clearance >= margin
// Lengthwise (yaw 0) the bar passes; crosswise (yaw 90) its ends come within the margin of the door posts.  Prints one line per
// yaw and one JSON line at the end, with the quaternions it used (a test that repeats the poses elsewhere need not repeat the
// sine and cosine); tests/test_cpp_body.py builds the same scene through the Python class and asserts that the numbers agree.
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
  const double margin = 0.1, pi = 3.14159265358979323846;
  const Eigen::Vector3d door(0.1, 0.0, 2.0);  // the middle of the doorway: the centre of the wall's voxel layer, half way up
  std::vector<Eigen::Vector3d> pos;
  std::vector<std::array<double, 4>> rot;
  for (int k = 0; k < 12; ++k) {
    const double half = 0.5 * (k * 15.0) * pi / 180.0;
    pos.push_back(door), rot.push_back({std::cos(half), 0.0, 0.0, std::sin(half)});
  }
  const fiesta::ESDFMap::BodyResult r = m.BodyQueryBatch(bar, pos, rot, margin);
  for (int k = 0; k < 12; ++k) {
    const bool free_scalar = m.IsPoseFree(bar, pos[k], rot[k], margin);
    std::printf("yaw %3d deg: %s  clearance %.3f m at sphere %d, %d spheres below the margin, cost %.4f, torque about z %.4f\n", k * 15,
                free_scalar ? "passes " : "blocked", r.min_clearance[k], r.min_sphere[k], r.n_below[k], r.cost[k], r.grad[k][5]);
    if (free_scalar != (r.min_clearance[k] >= margin)) return 1;
  }

  std::printf("{\"margin\": %.17g, \"position\": [%.17g, %.17g, %.17g], \"spheres\": [", margin, door(0), door(1), door(2));
  for (size_t i = 0; i < bar.size(); ++i) std::printf("%s[%.17g, %.17g, %.17g, %.17g]", i ? ", " : "", bar[i][0], bar[i][1], bar[i][2], bar[i][3]);
  std::printf("], \"poses\": [");
  for (int k = 0; k < 12; ++k) {
    std::printf("%s{\"yaw_deg\": %d, \"quat\": [%.17g, %.17g, %.17g, %.17g], \"passes\": %s, \"min_clearance\": %.17g, \"min_sphere\": %d, "
                "\"n_below\": %d, \"cost\": %.17g, \"grad\": [%.17g, %.17g, %.17g, %.17g, %.17g, %.17g]}",
                k ? ", " : "", k * 15, rot[k][0], rot[k][1], rot[k][2], rot[k][3], r.min_clearance[k] >= margin ? "true" : "false", r.min_clearance[k],
                r.min_sphere[k], r.n_below[k], r.cost[k], r.grad[k][0], r.grad[k][1], r.grad[k][2], r.grad[k][3], r.grad[k][4], r.grad[k][5]);
  }
  std::printf("]}\n");
  return 0;
}
