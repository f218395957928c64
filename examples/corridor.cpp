// examples/corridor.cpp -- "and where may the trajectory go?": the step after the reach paths, through the drop-in class
// (include/fiesta/ESDFMap.h), on the scene of examples/reach.cpp -- 40 x 40 x 20 voxels (0.2 m) seen through one view cone from voxel
// (5, 20, 10) along +x that ends on a wall at x = 30 and holds one pillar, and a pocket behind the wall that is out of reach.
//   GetFrontierVoxels   where known free space ends
//   ReachField          the travel cost from the robot's voxel to every one of them; the map retains the cost field
//   ReachPaths          the paths to all of them, pulled tight by line of sight
//   PathCorridor        per path the safe flight corridor: overlapping boxes of free space, what a trajectory optimiser fits a spline in
//   FreeBoxes           the free box around the robot itself
// Prints the corridor of the longest path and one JSON line at the end; tests/test_cpp_corridor.py builds the same scene through the
// Python class and asserts that the numbers agree.
#include <algorithm>
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
    if (cycle == 0)  // the pocket: 4 x 4 x 4 free voxels behind the wall
      for (int x = 33; x <= 36; ++x)
        for (int y = 18; y <= 21; ++y)
          for (int z = 8; z <= 11; ++z) m.SetOccupancy(Eigen::Vector3i(x, y, z), 0);
    m.UpdateOccupancy(true);
  }
  m.UpdateESDF();

  std::vector<Eigen::Vector3i> frontier;
  m.GetFrontierVoxels(0.0, frontier);
  // (the frontier call's order is unspecified: sort, so that path p is the same path on every run)
  std::sort(frontier.begin(), frontier.end(), [](const Eigen::Vector3i &a, const Eigen::Vector3i &b) {
    return a(0) != b(0) ? a(0) < b(0) : (a(1) != b(1) ? a(1) < b(1) : a(2) < b(2));
  });
  const std::vector<Eigen::Vector3i> robot{Eigen::Vector3i(sx + 7, sy, sz)};  // the robot has moved into the cone, in front of the pillar
  m.ReachField(nullptr, nullptr, robot, {}, 0.0, 26, 0, nullptr);
  const auto paths = m.ReachPaths(frontier, 26, true, 64);
  const int max_grow = 8;
  const auto cor = m.PathCorridor(paths.vox, paths.offsets, max_grow);
  const auto own = m.FreeBoxes(robot, max_grow);

  const size_t n = frontier.size();
  long long ok = 0, blocked = 0, invalid = 0, reached = 0, volume = 0, chain = 0;
  size_t longest = 0;
  for (size_t p = 0; p < n; ++p) {
    reached += paths.status[p] == FIESTA_HIP_REACH_PATH_OK;
    ok += cor.status[p] == FIESTA_HIP_CORRIDOR_OK, blocked += cor.status[p] == FIESTA_HIP_CORRIDOR_BLOCKED, invalid += cor.status[p] == FIESTA_HIP_CORRIDOR_INVALID;
    chain += cor.n_chain[p];
    if (cor.offsets[p + 1] - cor.offsets[p] > cor.offsets[longest + 1] - cor.offsets[longest]) longest = p;
  }
  const long long boxes = (long long)cor.offsets[n];
  for (long long k = 0; k < boxes; ++k) {
    const int32_t *b = &cor.boxes[6 * k];
    volume += (long long)(b[3] - b[0] + 1) * (b[4] - b[1] + 1) * (b[5] - b[2] + 1);
  }
  std::printf("%zu frontier voxels, %lld reached; %lld corridors OK, %lld boxes, %lld voxels in them\n", n, reached, ok, boxes, volume);
  std::printf("the corridor to (%d, %d, %d):\n", frontier[longest](0), frontier[longest](1), frontier[longest](2));
  for (int64_t k = cor.offsets[longest]; k < cor.offsets[longest + 1]; ++k)
    std::printf("  voxels (%d, %d, %d) .. (%d, %d, %d)   %.1f %.1f %.1f .. %.1f %.1f %.1f m, entered at chain voxel %d\n", cor.boxes[6 * k],
                cor.boxes[6 * k + 1], cor.boxes[6 * k + 2], cor.boxes[6 * k + 3], cor.boxes[6 * k + 4], cor.boxes[6 * k + 5], cor.pos[6 * k],
                cor.pos[6 * k + 1], cor.pos[6 * k + 2], cor.pos[6 * k + 3], cor.pos[6 * k + 4], cor.pos[6 * k + 5], cor.entry[k]);
  std::printf("{\"frontier\": %zu, \"reached\": %lld, \"ok\": %lld, \"blocked\": %lld, \"invalid\": %lld, \"boxes\": %lld, \"volume\": %lld, \"chain\": %lld, "
              "\"longest\": [%d, %d, %d], \"longest_boxes\": [",
              n, reached, ok, blocked, invalid, boxes, volume, chain, frontier[longest](0), frontier[longest](1), frontier[longest](2));
  for (int64_t k = cor.offsets[longest]; k < cor.offsets[longest + 1]; ++k)
    std::printf("%s[%d, %d, %d, %d, %d, %d]", k > cor.offsets[longest] ? ", " : "", cor.boxes[6 * k], cor.boxes[6 * k + 1], cor.boxes[6 * k + 2],
                cor.boxes[6 * k + 3], cor.boxes[6 * k + 4], cor.boxes[6 * k + 5]);
  std::printf("], \"robot_box\": [%d, %d, %d, %d, %d, %d], \"robot_volume\": %lld, \"robot_corner\": %.17g}\n", own.box[0], own.box[1], own.box[2], own.box[3],
              own.box[4], own.box[5], (long long)own.volume[0], own.pos[3]);
  return 0;
}
