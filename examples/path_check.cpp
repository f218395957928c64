// examples/path_check.cpp -- a planner's clearance check through the drop-in class (include/fiesta/ESDFMap.h): a small map with four
// pillars, then candidate paths asked as whole polylines instead of sample by sample.
//   GetMinDistanceAlongPath   one path (here <= 256 samples: answered from the host brick cache)
//   PathClearanceBatch        several paths in CSR form (here on the GPU)
//   PathSample                a sample index back to its position, on the host
// Prints one JSON line; doubles as hex strings ("%a": exact).  Built with plain g++ against libfiesta_hip.so
// (tests/test_gpu_path_queries.py compares it with the Python mirror); build it with -ffp-contract=off, as PathSample asks.
#include <cstdio>
#include <vector>

#include "fiesta/ESDFMap.h"

static void hex(const char *key, const double *v, int n, const char *tail) {
  std::printf("\"%s\": [", key);
  for (int i = 0; i < n; ++i) std::printf("\"%a\"%s", v[i], i + 1 < n ? ", " : "");
  std::printf("]%s", tail);
}

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

  // one path, the facade's single call: 3.5 m at 0.05 m -> 71 samples, host side
  const std::vector<Eigen::Vector3d> one{Eigen::Vector3d(-3.0, -2.0, 1.0), Eigen::Vector3d(-1.5, -1.0, 1.1),
                                         Eigen::Vector3d(0.5, -1.9, 1.2)};
  Eigen::Vector3d grad, fbp;
  int64_t fb = -1;
  const double md = m.GetMinDistanceAlongPath(one, 0.05, 0.5, &grad, &fb, &fbp);

  // three paths in one batch: a diagonal through the pillars, a zig-zag, one that leaves the map (contact where it leaves)
  const double w[] = {-3.5, -3.5, 1.0, 3.5, 3.5, 1.0,
                      -3.0, 2.0, 0.5, -1.0, -2.0, 1.5, 1.0, 2.0, 2.5, 2.0, -3.0, 3.5, 3.0, 0.0, 0.3,
                      0.0, 0.0, 2.0, 2.0, 1.0, 2.0, 6.0, 1.0, 2.0};
  const int64_t off[] = {0, 2, 7, 10};
  double min_dist[3], min_pos[9], min_grad[9], fb_pos[9];
  int64_t min_index[3], first_below[3], n_samples[3];
  const fiesta_hip_path_result r{min_dist, min_index, min_pos, min_grad, first_below, fb_pos, n_samples};
  m.PathClearanceBatch(w, 10, off, 3, 0.05, 0.5, r);

  // the batch's minima mapped back to positions on the host
  double back[9];
  for (int p = 0; p < 3; ++p) {
    std::vector<Eigen::Vector3d> path;
    for (int64_t i = off[p]; i < off[p + 1]; ++i) path.push_back(Eigen::Vector3d(w[3 * i], w[3 * i + 1], w[3 * i + 2]));
    const Eigen::Vector3d s = fiesta::ESDFMap::PathSample(path, 0.05, min_index[p]);
    for (int c = 0; c < 3; ++c) back[3 * p + c] = s(c);
  }

  std::printf("{");
  hex("one_min_dist", &md, 1, ", ");
  const double g[3] = {grad(0), grad(1), grad(2)}, f[3] = {fbp(0), fbp(1), fbp(2)};
  hex("one_min_grad", g, 3, ", ");
  std::printf("\"one_first_below\": %lld, ", (long long)fb);
  hex("one_first_below_pos", f, 3, ", ");
  hex("min_dist", min_dist, 3, ", ");
  hex("min_pos", min_pos, 9, ", ");
  hex("min_grad", min_grad, 9, ", ");
  hex("first_below_pos", fb_pos, 9, ", ");
  hex("path_sample_of_min", back, 9, ", ");
  std::printf("\"min_index\": [%lld, %lld, %lld], ", (long long)min_index[0], (long long)min_index[1], (long long)min_index[2]);
  std::printf("\"first_below\": [%lld, %lld, %lld], ", (long long)first_below[0], (long long)first_below[1], (long long)first_below[2]);
  std::printf("\"n_samples\": [%lld, %lld, %lld]}\n", (long long)n_samples[0], (long long)n_samples[1], (long long)n_samples[2]);
  return 0;
}
