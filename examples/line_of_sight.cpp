// examples/line_of_sight.cpp -- the ray questions of a planner through the drop-in class (include/fiesta/ESDFMap.h), on the scene of
// examples/frontiers.cpp: a room of 40 x 40 x 20 voxels (0.2 m) seen through ONE view cone -- sensor at voxel (5, 20, 10) looking
// along +x -- that ends on a wall at x = 30 and holds one pillar; everything outside the cone was never observed.
//   RayQueryBatch   a fan of rays from the sensor through the wall, and segments between points inside the room: with stop_mask 7
//                   (occupied, unknown and outside all block) the line-of-sight test of path shortcutting; with stop_mask 1 the
//                   expected depth (hit_dist) and the information gain (unknown voxels before the first obstacle)
//   RayQuery        one ray, the same answer
//   IsSegmentFree   valid and nothing but voxels observed free
// Prints a summary and one JSON line at the end; tests/test_cpp_ray_queries.py runs the same rays through the Python class and
// asserts that the numbers agree.
#include <cmath>
#include <cstdio>
#include <vector>

#include "fiesta/ESDFMap.h"

static Eigen::Vector3d centre(double x, double y, double z) {  // the centre of voxel (x, y, z); fractions: a point inside it
  return Eigen::Vector3d(-4.0 + (x + 0.5) * 0.2, -4.0 + (y + 0.5) * 0.2, 0.0 + (z + 0.5) * 0.2);
}

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
    m.UpdateOccupancy(true);
  }
  // (no UpdateESDF: the classes of a ray query follow UpdateOccupancy, the distance field is not read)

  std::vector<Eigen::Vector3d> from, to;
  for (int y = 2; y <= 38; y += 3)  // a fan from just in front of the sensor to a plane behind the wall
    for (int z = 1; z <= 19; z += 3) from.push_back(centre(sx + 1, sy, sz)), to.push_back(centre(36, y, z));
  for (int y = 12; y <= 28; y += 2) {  // segments across the room, in front of and behind the pillar
    from.push_back(centre(12.25, y, 10.25)), to.push_back(centre(26.5, 40 - y, 9.75));
    from.push_back(centre(22, y, 6)), to.push_back(centre(28, y, 14));
  }
  from.push_back(centre(10, 20, 10)), to.push_back(centre(45, 20, 10));  // through the pillar and out of the map
  from.push_back(centre(8, 20, 10)), to.push_back(centre(8, 20, 10));    // zero length
  const int64_t n = (int64_t)from.size();
  std::vector<double> a(3 * n), b(3 * n);
  for (int64_t i = 0; i < n; ++i)
    for (int c = 0; c < 3; ++c) a[3 * i + c] = from[i](c), b[3 * i + c] = to[i](c);

  std::vector<int32_t> hit_index(n), n_visited(n), counts(4 * n), gain_counts(4 * n), vox(3 * n);
  std::vector<uint8_t> hit_class(n);
  std::vector<double> depth(n);
  fiesta_hip_ray_result los{};
  los.hit_index = hit_index.data(), los.hit_class = hit_class.data(), los.n_visited = n_visited.data(), los.counts = counts.data(),
  los.hit_vox = vox.data();
  m.RayQueryBatch(a.data(), b.data(), n, 7, los);
  fiesta_hip_ray_result view{};
  view.hit_dist = depth.data(), view.counts = gain_counts.data();
  m.RayQueryBatch(a.data(), b.data(), n, FIESTA_HIP_RAY_OCCUPIED, view);

  int clear = 0, by_class[5] = {0, 0, 0, 0, 0}, agree = 1;
  long gain = 0, depth_mm = 0;
  for (int64_t i = 0; i < n; ++i) {
    const fiesta::ESDFMap::RayHit h = m.RayQuery(from[i], to[i], 7);
    agree &= h.n_visited == n_visited[i] && h.hit_index == hit_index[i] && h.hit_class == hit_class[i] && h.counts[0] == counts[4 * i] &&
             h.counts[2] == counts[4 * i + 2] && (!h.hit() || (h.hit_vox(0) == vox[3 * i] && h.hit_vox(1) == vox[3 * i + 1] && h.hit_vox(2) == vox[3 * i + 2]));
    agree &= m.IsSegmentFree(from[i], to[i]) == (n_visited[i] >= 0 && hit_index[i] < 0);
    const fiesta::ESDFMap::RayHit d = m.RayQuery(from[i], to[i], FIESTA_HIP_RAY_OCCUPIED);
    agree &= (std::isnan(d.hit_dist) && std::isnan(depth[i])) || d.hit_dist == depth[i];
    if (hit_index[i] < 0) ++clear;
    ++by_class[hit_class[i]];
    gain += gain_counts[4 * i + 2];
    if (!std::isnan(depth[i])) depth_mm += std::lround(depth[i] * 1000.0);
  }
  agree &= !m.IsSegmentFree(Eigen::Vector3d(std::nan(""), 0, 0), centre(8, 20, 10));  // an invalid ray is not free
  std::printf("%lld rays: %d clear, blocked by occupied %d, unknown %d, outside %d\n", (long long)n, clear, by_class[1], by_class[2], by_class[4]);
  std::printf("  unknown voxels before the first obstacle: %ld; sum of expected depths: %ld mm\n", gain, depth_mm);
  std::printf("  one-ray calls and IsSegmentFree agree with the batch: %s\n", agree ? "yes" : "NO");
  std::printf("{\"rays\": %lld, \"clear\": %d, \"occupied\": %d, \"unknown\": %d, \"outside\": %d, \"gain\": %ld, \"depth_mm\": %ld, \"agree\": %d}\n",
              (long long)n, clear, by_class[1], by_class[2], by_class[4], gain, depth_mm, agree);
  return agree ? 0 : 1;
}
