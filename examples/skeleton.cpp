// examples/skeleton.cpp -- "where is the middle of the passage, and how narrow is it?" through the drop-in class
// (include/fiesta/ESDFMap.h): the map of examples/frontiers.cpp, fully observed, cut into two rooms by two walls in the plane x = 20
// that leave a doorway four voxels wide between them.
//   GetSkeletonVoxels   the free voxels on the distance field's ridge: a neighbour's closest obstacle lies at least 3 voxels from
//                       the voxel's own and the bisector of the two passes between them -- here the sheet half way between the two
//                       door posts, through the doorway and on into both rooms
//   ClusterVoxels       the connected pieces of the skeleton; with key = d2 each piece comes with its NARROWEST member: the
//                       bottleneck of the passage (clearance sqrt(d2) voxels on either side)
// The skeleton call's order is unspecified and cluster ids follow the list's order, so the list is sorted first: the output is the
// same on every run.  Prints the clusters and one JSON line at the end; tests/test_cpp_skeleton.py builds the same scene through the
// Python class and asserts that the numbers agree.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <numeric>
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

  const int32_t min_sep2 = 9;
  const fiesta::ESDFMap::SkeletonVoxels found = m.GetSkeletonVoxels(nullptr, nullptr, min_sep2);
  std::vector<size_t> order(found.count());
  std::iota(order.begin(), order.end(), (size_t)0);
  std::sort(order.begin(), order.end(), [&](size_t i, size_t j) {
    const auto &a = found.vox[i], &b = found.vox[j];
    return a(0) != b(0) ? a(0) < b(0) : (a(1) != b(1) ? a(1) < b(1) : a(2) < b(2));
  });
  fiesta::ESDFMap::SkeletonVoxels sk;
  for (size_t i : order) sk.vox.push_back(found.vox[i]), sk.mask.push_back(found.mask[i]), sk.d2.push_back(found.d2[i]), sk.sep2.push_back(found.sep2[i]);

  const int32_t min_size = 5;
  const fiesta::ESDFMap::VoxelClusters c = m.ClusterVoxels(sk.vox, &sk.mask, &sk.d2, 26, min_size);
  std::printf("skeleton voxels: %zu in %lld clusters of at least %d (%lld smaller ones dropped), largest %lld\n", sk.count(),
              (long long)c.info.n_clusters, min_size, (long long)c.info.n_dropped_clusters, (long long)c.info.largest);
  for (size_t k = 0; k < c.count(); ++k) {
    const auto &v = sk.vox[(size_t)c.key_argmin[k]];
    std::printf("  cluster %zu: %d voxels, box (%d, %d, %d) .. (%d, %d, %d), narrowest at (%d, %d, %d): %.2f m to the nearest obstacle\n", k, c.size[k],
                c.box_lo[k](0), c.box_lo[k](1), c.box_lo[k](2), c.box_hi[k](0), c.box_hi[k](1), c.box_hi[k](2), v(0), v(1), v(2),
                std::sqrt((double)c.key_min[k]) * 0.2);
  }

  std::printf("{\"skeleton\": %zu, \"n_clusters\": %lld, \"n_dropped_clusters\": %lld, \"n_members\": %lld, \"largest\": %lld, \"clusters\": [",
              sk.count(), (long long)c.info.n_clusters, (long long)c.info.n_dropped_clusters, (long long)c.info.n_members, (long long)c.info.largest);
  for (size_t k = 0; k < c.count(); ++k) {
    const auto &v = sk.vox[(size_t)c.key_argmin[k]];
    std::printf("%s{\"size\": %d, \"root\": %lld, \"box_lo\": [%d, %d, %d], \"box_hi\": [%d, %d, %d], \"mask_or\": %d, \"key_min\": %d, "
                "\"key_argmin\": %lld, \"narrowest\": [%d, %d, %d], \"sep2\": %d}",
                k ? ", " : "", c.size[k], (long long)c.root[k], c.box_lo[k](0), c.box_lo[k](1), c.box_lo[k](2), c.box_hi[k](0), c.box_hi[k](1),
                c.box_hi[k](2), (int)c.mask_or[k], c.key_min[k], (long long)c.key_argmin[k], v(0), v(1), v(2), sk.sep2[(size_t)c.key_argmin[k]]);
  }
  std::printf("]}\n");
  return 0;
}
