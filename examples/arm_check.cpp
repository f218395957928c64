// examples/arm_check.cpp -- "which shoulder angles let the arm reach through the door?" through the drop-in class
// (include/fiesta/ESDFMap.h): the doorway scene of examples/body_check.cpp -- two rooms, two walls in the plane x = 20 voxels that
// leave a doorway four voxels (0.8 m) wide.  A planar three-link arm stands 0.85 m in front of the middle of the doorway: two links
// of 0.4 m with three spheres of radius 0.1 m each, a hand of 0.25 m with two spheres of radius 0.08 m.  Every link is a FRAME: its
// origin is the joint it hangs on, its x axis runs along the link.  The elbow and the wrist are bent by 15 degrees each; the shoulder
// sweeps 12 angles, 10 degrees apart.  The forward kinematics is done here, once: the call takes the frame poses.
//   ArticulatedQueryBatch   per configuration the clearance of the closest sphere and which sphere that is, the obstacle penalty, and
//                           per link its own clearance, penalty, force and torque
//   IsConfigurationFree     the scalar convenience: min_clearance >= margin
// Straight at the doorway the arm reaches through; swung to either side the hand meets a door post, and further out it is clear of
// the wall again.  Prints one line per angle and one JSON line at the end, with the frame poses it used (a test that repeats the
// configurations elsewhere need not repeat the sines and cosines); tests/test_cpp_articulated.py builds the same scene through the
// Python class and asserts that the numbers agree.
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

  const int F = 3, N = 12;
  const double length[F] = {0.4, 0.4, 0.25};
  fiesta::ESDFMap::BodySpheres spheres;
  std::vector<int32_t> sphere_frame;
  for (int f = 0; f < F; ++f)
    for (int i = 0; i < (f < 2 ? 3 : 2); ++i) spheres.push_back({0.05 + 0.15 * i, 0.0, 0.0, f < 2 ? 0.1 : 0.08}), sphere_frame.push_back(f);
  const double margin = 0.1, pi = 3.14159265358979323846, deg = pi / 180.0;
  const double base[3] = {-0.75, 0.0, 2.0};  // the shoulder: 0.85 m in front of the wall's voxel layer, half way up
  const double elbow = 15.0 * deg, wrist = 15.0 * deg;
  std::vector<double> poses;  // N x F x 7
  for (int k = 0; k < N; ++k) {
    const double shoulder = (-60.0 + 10.0 * k) * deg;
    const double heading[F] = {shoulder, shoulder + elbow, shoulder + elbow + wrist};
    double joint[3] = {base[0], base[1], base[2]};
    for (int f = 0; f < F; ++f) {
      const double pose[7] = {joint[0], joint[1], joint[2], std::cos(0.5 * heading[f]), 0.0, 0.0, std::sin(0.5 * heading[f])};
      poses.insert(poses.end(), pose, pose + 7);
      joint[0] += length[f] * std::cos(heading[f]), joint[1] += length[f] * std::sin(heading[f]);
    }
  }
  const fiesta::ESDFMap::ArticulatedResult r = m.ArticulatedQueryBatch(spheres, sphere_frame, F, poses, margin);
  for (int k = 0; k < N; ++k) {
    const std::vector<double> one(poses.begin() + 7 * F * k, poses.begin() + 7 * F * (k + 1));
    const bool free_scalar = m.IsConfigurationFree(spheres, sphere_frame, F, one, margin);
    std::printf("shoulder %4d deg: %s  clearance %.3f m at sphere %d (link %d), %d spheres below the margin, cost %.4f, link clearances %.3f %.3f %.3f\n",
                -60 + 10 * k, free_scalar ? "passes " : "blocked", r.min_clearance[k], r.min_sphere[k], sphere_frame[r.min_sphere[k]], r.n_below[k],
                r.cost[k], r.frame_clearance[F * k], r.frame_clearance[F * k + 1], r.frame_clearance[F * k + 2]);
    if (free_scalar != (r.min_clearance[k] >= margin)) return 1;
  }

  std::printf("{\"margin\": %.17g, \"n_frames\": %d, \"spheres\": [", margin, F);
  for (size_t i = 0; i < spheres.size(); ++i)
    std::printf("%s[%.17g, %.17g, %.17g, %.17g]", i ? ", " : "", spheres[i][0], spheres[i][1], spheres[i][2], spheres[i][3]);
  std::printf("], \"sphere_frame\": [");
  for (size_t i = 0; i < sphere_frame.size(); ++i) std::printf("%s%d", i ? ", " : "", sphere_frame[i]);
  std::printf("], \"configurations\": [");
  for (int k = 0; k < N; ++k) {
    std::printf("%s{\"shoulder_deg\": %d, \"frame_poses\": [", k ? ", " : "", -60 + 10 * k);
    for (int f = 0; f < F; ++f) {
      const double *p = &poses[7 * (F * k + f)];
      std::printf("%s[%.17g, %.17g, %.17g, %.17g, %.17g, %.17g, %.17g]", f ? ", " : "", p[0], p[1], p[2], p[3], p[4], p[5], p[6]);
    }
    std::printf("], \"passes\": %s, \"min_clearance\": %.17g, \"min_sphere\": %d, \"n_below\": %d, \"cost\": %.17g, \"frame_clearance\": [%.17g, %.17g, %.17g], "
                "\"frame_cost\": [%.17g, %.17g, %.17g], \"frame_grad\": [",
                r.min_clearance[k] >= margin ? "true" : "false", r.min_clearance[k], r.min_sphere[k], r.n_below[k], r.cost[k], r.frame_clearance[F * k],
                r.frame_clearance[F * k + 1], r.frame_clearance[F * k + 2], r.frame_cost[F * k], r.frame_cost[F * k + 1], r.frame_cost[F * k + 2]);
    for (int f = 0; f < F; ++f) {
      const std::array<double, 6> &g = r.frame_grad[F * k + f];
      std::printf("%s[%.17g, %.17g, %.17g, %.17g, %.17g, %.17g]", f ? ", " : "", g[0], g[1], g[2], g[3], g[4], g[5]);
    }
    std::printf("]}");
  }
  std::printf("]}\n");
  return 0;
}
