// examples/frontier_split.cpp -- "where do the viewpoints go?" through the drop-in class (include/fiesta/ESDFMap.h): the scene of
// examples/reach.cpp -- a room seen through one view cone that ends on a wall and holds a pillar, and a pocket of free space behind
// the wall that touches the cone nowhere.
//   GetFrontierVoxels   where known free space ends: single voxels
//   ClusterVoxels       the FRONTIERS: connected groups of those voxels -- the mantle of the cone is ONE of them, thousands of voxels
//                       around a centroid that lies in the middle of the room and sees none of them
//   SplitClusters       view-sized PARTS: every part with more than max_size voxels or longer than max_extent is cut at the middle of
//                       its box's longest axis; each part has its own size, box and centroid
// The frontier call's order is unspecified and cluster ids follow the list's order, so the list is sorted first: the output is the
// same on every run.  Prints the parts and one JSON line at the end; tests/test_cpp_split.py builds the same scene through the
// Python class and asserts that the numbers agree.
#include <algorithm>
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

  const int32_t min_size = 5, max_size = 96, max_extent = 12;
  const fiesta::ESDFMap::VoxelClusters c = m.ClusterVoxels(frontier, &mask, nullptr, 26, min_size);
  const fiesta::ESDFMap::ClusterParts p = m.SplitClusters(frontier, c.offsets, c.members, &mask, nullptr, max_size, max_extent);
  std::printf("frontier voxels: %zu in %lld clusters (largest %lld) -> %lld parts of at most %d voxels and %d across (largest %lld, %lld "
              "clusters cut, deepest level %lld)\n",
              frontier.size(), (long long)c.info.n_clusters, (long long)c.info.largest, (long long)p.info.n_parts, max_size, max_extent,
              (long long)p.info.largest, (long long)p.info.n_split_clusters, (long long)p.info.depth);
  unsigned long long checksum = 1469598103934665603ull;  // FNV-1a over (parent, depth, size, root, box) of every part, in part order
  const auto mix = [&](long long x) {
    for (int b = 0; b < 8; ++b) checksum = (checksum ^ ((unsigned long long)x >> (8 * b) & 0xFFull)) * 1099511628211ull;
  };
  for (size_t k = 0; k < p.count(); ++k) {
    if (k < 12)
      std::printf("  part %zu of cluster %d (depth %d): %d voxels, box (%d, %d, %d) .. (%d, %d, %d), centroid (%.3f, %.3f, %.3f) m\n", k, p.parent[k],
                  (int)p.depth[k], p.size[k], p.box_lo[k](0), p.box_lo[k](1), p.box_lo[k](2), p.box_hi[k](0), p.box_hi[k](1), p.box_hi[k](2),
                  p.centroid[k](0), p.centroid[k](1), p.centroid[k](2));
    mix(p.parent[k]), mix(p.depth[k]), mix(p.size[k]), mix(p.root[k]);
    for (int a = 0; a < 3; ++a) mix(p.box_lo[k](a)), mix(p.box_hi[k](a));
  }

  std::printf("{\"frontier\": %zu, \"n_clusters\": %lld, \"n_parts\": %lld, \"n_members\": %lld, \"n_split_clusters\": %lld, \"n_oversize\": %lld, "
              "\"largest\": %lld, \"depth\": %lld, \"status\": %lld, \"checksum\": %llu, \"sizes\": [",
              frontier.size(), (long long)c.info.n_clusters, (long long)p.info.n_parts, (long long)p.info.n_members, (long long)p.info.n_split_clusters,
              (long long)p.info.n_oversize, (long long)p.info.largest, (long long)p.info.depth, (long long)p.info.status, checksum);
  for (size_t k = 0; k < p.count(); ++k) std::printf("%s%d", k ? ", " : "", p.size[k]);
  std::printf("], \"parents\": [");
  for (size_t k = 0; k < p.count(); ++k) std::printf("%s%d", k ? ", " : "", p.parent[k]);
  std::printf("], \"centroids\": [");
  for (size_t k = 0; k < p.count(); ++k) std::printf("%s[%.17g, %.17g, %.17g]", k ? ", " : "", p.centroid[k](0), p.centroid[k](1), p.centroid[k](2));
  std::printf("]}\n");
  return 0;
}
