// examples/frontiers.cpp -- the map-side question of an exploration planner through the drop-in class (include/fiesta/ESDFMap.h):
// a room of 40 x 40 x 20 voxels (0.2 m) seen through ONE view cone -- sensor at voxel (5, 20, 10) looking along +x, 45 degrees half
// angle, 5.6 m range -- that ends on a wall at x = 30 and holds one pillar; everything outside the cone was never observed.
//   GetFrontierVoxels   the observed-free voxels that border unknown space, with their unknown-neighbour masks; a second call keeps
//                       only those at least 0.3 m from every obstacle (where a robot of that radius can stand), a third is
//                       restricted to a box, as a planner does with the bounding box of the last sensor frame
// Prints the three counts and one JSON line at the end; tests/test_gpu_frontiers.py builds the same scene through the Python class
// and asserts that the counts agree.
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
    m.UpdateOccupancy(true);
  }
  m.UpdateESDF();

  std::vector<Eigen::Vector3i> all, clear, boxed;
  std::vector<uint8_t> mask;
  m.GetFrontierVoxels(0.0, all, &mask);
  m.GetFrontierVoxels(0.3, clear);
  m.GetFrontierVoxels(Eigen::Vector3i(6, 0, 0), Eigen::Vector3i(17, 39, 19), 0.0, boxed);
  int faces = 0;
  for (uint8_t u : mask)
    for (int b = 0; b < 6; ++b) faces += (u >> b) & 1;
  std::printf("frontier voxels: %zu (%d faces towards unknown space)\n", all.size(), faces);
  std::printf("  with 0.3 m clearance: %zu\n", clear.size());
  std::printf("  inside the box x = 6 .. 17: %zu\n", boxed.size());
  std::printf("{\"frontier\": %zu, \"faces\": %d, \"clear\": %zu, \"boxed\": %zu}\n", all.size(), faces, clear.size(), boxed.size());
  return 0;
}
