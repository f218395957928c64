// examples/frontier_views.cpp -- "where do I look at that frontier from?" through the drop-in class (include/fiesta/ESDFMap.h): the
// scene of examples/frontier_clusters.cpp -- a room seen through one view cone that ends on a wall and holds a pillar, and a pocket of
// free space behind the wall.
//   GetFrontierVoxels   where known free space ends: single voxels
//   ClusterVoxels       the FRONTIERS: connected groups of those voxels with their centroids and member lists
//   ViewCoverage        a ring of candidate poses around every centroid (2 radii x 12 angles, looking inwards) against the cluster's own
//                       voxels: a camera of 80 x 60 degrees and 3 m range that stands at least 0.3 m from obstacles and sees nothing
//                       behind occupied or never-observed voxels; per cluster the pose that sees most of it
//   GetFrontierViews    the three calls composed (on the frontier call's own order: the same clusters under other numbers)
// The frontier call's order is unspecified and cluster ids follow the list's order, so the list is sorted first: the output is the
// same on every run.  Prints the clusters and one JSON line at the end; tests/test_cpp_views.py builds the same scene through the
// Python class and asserts that the numbers agree.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <numeric>
#include <utility>
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

  const int32_t min_size = 5;
  const fiesta::ESDFMap::VoxelClusters c = m.ClusterVoxels(frontier, &mask, nullptr, 26, min_size);
  const std::vector<fiesta::ESDFMap::RingRow> ring = fiesta::ESDFMap::ViewRing({0.8, 1.6}, 12, {0.0});
  const double deg = 3.141592653589793 / 180.0;
  const fiesta_hip_view_sensor cam = fiesta::ESDFMap::ViewSensor(0.2, 3.0, std::tan(40.0 * deg), std::tan(30.0 * deg),
                                                                 FIESTA_HIP_RAY_OCCUPIED | FIESTA_HIP_RAY_UNKNOWN, false, 0.3, 3);
  const fiesta::ESDFMap::ViewCoverageResult v = m.ViewCoverage(frontier, c.centroid, ring, cam, &c.offsets, &c.members);
  std::printf("frontier voxels: %zu in %zu clusters; %zu candidate views, %lld usable, %lld pairs, %lld in view, %lld visible\n", frontier.size(),
              c.count(), v.n_visible.size(), (long long)v.info.n_usable, (long long)v.info.n_pairs, (long long)v.info.n_in_view,
              (long long)v.info.n_visible);
  for (size_t k = 0; k < c.count(); ++k) {
    std::printf("  cluster %zu: %d voxels around (%.2f, %.2f, %.2f) m", k, c.size[k], c.centroid[k](0), c.centroid[k](1), c.centroid[k](2));
    if (v.best_view[k] >= 0) {
      const auto &r = ring[(size_t)v.best_view[k] % ring.size()];
      std::printf(": best seen from (%.2f, %.2f, %.2f) m looking along (%.2f, %.2f), %d of its voxels\n", c.centroid[k](0) + r[0],
                  c.centroid[k](1) + r[1], c.centroid[k](2) + r[2], r[3], r[4], v.best_count[k]);
    } else {
      std::printf(": no pose of the ring sees %d of its voxels\n", cam.min_visible);
    }
  }
  size_t unseen = 0;
  for (int32_t n : v.cover_count) unseen += n == 0;
  std::printf("  %zu frontier voxels are seen by no candidate\n", unseen);

  // the composed call works on the frontier call's own order: the same clusters, numbered differently
  std::vector<Eigen::Vector3i> vox2;
  const fiesta::ESDFMap::FrontierViewSet f = m.GetFrontierViews(nullptr, nullptr, 0.0, 26, min_size, ring, cam, vox2);
  std::vector<std::pair<int, int>> a, b;
  for (size_t k = 0; k < c.count(); ++k) a.push_back({c.size[k], v.best_count[k]});
  for (size_t k = 0; k < f.clusters.count(); ++k) b.push_back({f.clusters.size[k], f.coverage.best_count[k]});
  std::sort(a.begin(), a.end()), std::sort(b.begin(), b.end());
  const bool chain_ok = a == b && f.coverage.info.n_visible == v.info.n_visible && f.best_pos.size() == c.count();

  std::printf("{\"frontier\": %zu, \"n_clusters\": %zu, \"n_usable\": %lld, \"n_pairs\": %lld, \"pairs_in_view\": %lld, \"pairs_visible\": %lld, "
              "\"unseen\": %zu, \"chain_ok\": %s, \"ring\": [",
              frontier.size(), c.count(), (long long)v.info.n_usable, (long long)v.info.n_pairs, (long long)v.info.n_in_view,
              (long long)v.info.n_visible, unseen, chain_ok ? "true" : "false");
  for (size_t j = 0; j < ring.size(); ++j)
    std::printf("%s[%.17g, %.17g, %.17g, %.17g, %.17g]", j ? ", " : "", ring[j][0], ring[j][1], ring[j][2], ring[j][3], ring[j][4]);
  std::printf("], \"sensor\": [%.17g, %.17g, %.17g, %.17g, %.17g], \"best_view\": [", cam.min_range, cam.max_range, cam.tan_h, cam.tan_v, cam.min_clearance);
  for (size_t k = 0; k < c.count(); ++k) std::printf("%s%lld", k ? ", " : "", (long long)v.best_view[k]);
  std::printf("], \"best_count\": [");
  for (size_t k = 0; k < c.count(); ++k) std::printf("%s%d", k ? ", " : "", v.best_count[k]);
  std::printf("], \"n_visible\": [");
  for (size_t i = 0; i < v.n_visible.size(); ++i) std::printf("%s%d", i ? ", " : "", v.n_visible[i]);
  std::printf("], \"cover_count\": [");
  for (size_t i = 0; i < v.cover_count.size(); ++i) std::printf("%s%d", i ? ", " : "", v.cover_count[i]);
  std::printf("]}\n");
  return chain_ok ? 0 : 1;
}
