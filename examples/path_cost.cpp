// examples/path_cost.cpp -- the optimiser half of a planner through the drop-in class (include/fiesta/ESDFMap.h): a small map with
// four pillars, a straight path that grazes one of them inside the safety margin, and plain gradient descent on its interior
// waypoints (the end points stay) with the cost and the waypoint gradients of ONE call per iteration:
//   GetPathCost     the obstacle cost of the polyline and d cost / d waypoint (here about 600 samples per call: on the GPU)
// Prints the cost before every descent step and after the last one, one JSON line at the end.  With the fixed step size below the
// cost falls monotonically from 0.2804 to 0.0238 in 40 steps (the path bends around the pillar until it leaves the margin almost
// everywhere); tests/test_gpu_path_cost.py asserts that it never rises after the first step and ends below half of where it began.
#include <cstdio>
#include <vector>

#include "fiesta/ESDFMap.h"

int main() {
  fiesta::ESDFMap m(Eigen::Vector3d(-4.0, -4.0, 0.0), 0.2, Eigen::Vector3d(8.0, 8.0, 4.0));  // 40 x 40 x 20 voxels
  m.SetParameters(0.70, 0.35, 0.12, 0.97, 0.80);
  m.SetOriginalRange();
  for (int x = 0; x < 40; ++x)
    for (int y = 0; y < 40; ++y)
      for (int z = 0; z < 20; ++z) m.SetOccupancy(Eigen::Vector3i(x, y, z), 0);
  m.UpdateOccupancy(true);
  m.UpdateESDF();
  const int pillars[4][2] = {{10, 10}, {20, 25}, {30, 12}, {14, 31}};
  for (int cycle = 0; cycle < 3; ++cycle) {
    for (const auto &p : pillars)
      for (int z = 0; z < 20; ++z) m.SetOccupancy(Eigen::Vector3i(p[0], p[1], z), 1);
    m.UpdateOccupancy(true);
  }
  m.UpdateESDF();

  // 12 waypoints from (-2.6, 1.5, 1.0) to (2.9, 1.6, 1.0): 0.4 m beside the pillar at (0.1, 1.1), margin 1.0 m
  const int K = 12;
  const double step = 0.01, margin = 1.0, rate = 0.25;
  const int iterations = 40;
  std::vector<Eigen::Vector3d> path(K), grad;
  for (int i = 0; i < K; ++i) {
    const double t = (double)i / (K - 1);
    path[i] = Eigen::Vector3d(-2.6 + 5.5 * t, 1.5 + 0.1 * t, 1.0);
  }
  std::vector<double> costs;
  int64_t n_below = 0;
  for (int it = 0; it <= iterations; ++it) {
    const double cost = m.GetPathCost(path, step, margin, &grad, &n_below);
    costs.push_back(cost);
    std::printf("step %2d  cost %.6f  samples below the margin %lld\n", it, cost, (long long)n_below);
    if (it == iterations) break;
    for (int i = 1; i + 1 < K; ++i) path[i] = path[i] - grad[i] * rate;
  }
  std::printf("{\"costs\": [");
  for (size_t i = 0; i < costs.size(); ++i) std::printf("%.17g%s", costs[i], i + 1 < costs.size() ? ", " : "");
  std::printf("], \"final_path\": [");
  for (int i = 0; i < K; ++i) std::printf("[%.17g, %.17g, %.17g]%s", path[i](0), path[i](1), path[i](2), i + 1 < K ? ", " : "");
  std::printf("]}\n");
  return 0;
}
