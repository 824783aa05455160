// DenseSLAMSystem::collidesWith (se_hip_collide_boxes_host) against the host se::Octree that getMap() builds from the same device map:
// SE_HIP_COLLIDE_REFERENCE box for box with se::geometry::collides_with (include/se/octree_collision.hpp, the literal traversal), and
// SE_HIP_COLLIDE_STRICT with a brute-force min over Octree::get.  Drives the mirror over a SLAMBench .raw stream with ground-truth poses,
// the way examples/denseslam_raw.cpp does.
//   usage: collision_mirror <scene.raw> <poses.bin> <volume_res> <volume_dim> <mu>
// Prints one line: "checked <n> occupied <n> unseen <n> empty <n> differ <n> bad <n>" (counts of the reference answers; differ = boxes
// whose two modes disagree).
#include "mirror_scene.hpp"
#include <se/octree_collision.hpp>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <type_traits>
#include <vector>

int main(int argc, char** argv) {
  MirrorScene scene;
  if (int rc = scene.replay(argc, argv, 6, "scene.raw poses.bin res dim mu")) return rc;
  DenseSLAMSystem& pipeline = *scene.pipeline;
  const int res = scene.res;
  std::shared_ptr<se::Octree<FieldType> > map;
  const auto t_map = std::chrono::steady_clock::now();
  pipeline.getMap(map);
  const double getmap_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_map).count();
  if (map->getBlockBuffer().empty()) { std::fprintf(stderr, "empty map\n"); return 3; }

  // boxes (voxel units): uniform, around allocated blocks (the block's corner +- a few voxels), partly outside the volume, large
  const bool ofusion = std::is_same<FieldType, OFusion>::value;
  const se_hip_collide_test test = {0.f, ofusion ? 1 : 0};
  const se::geometry::voxel_test<FieldType> host_test = {0.f, ofusion};
  std::mt19937 rng(23);
  std::vector<int32_t> boxes;
  auto add = [&](int x, int y, int z, int a, int b, int c) { const int32_t v[6] = {x, y, z, a, b, c}; boxes.insert(boxes.end(), v, v + 6); };
  auto side = [&](int hi) { return 1 + (int)(rng() % (unsigned)hi); };
  for (int i = 0; i < 600; ++i) add((int)(rng() % (unsigned)(res + 32)) - 16, (int)(rng() % (unsigned)(res + 32)) - 16, (int)(rng() % (unsigned)(res + 32)) - 16, side(24), side(24), side(24));
  const auto& blocks = map->getBlockBuffer();
  for (int i = 0; i < 1400; ++i) {
    const int* c = blocks[rng() % blocks.size()]->coordinates();
    add(c[0] + (int)(rng() % 20) - 10, c[1] + (int)(rng() % 20) - 10, c[2] + (int)(rng() % 20) - 10, side(12), side(12), side(12));
  }
  for (int i = 0; i < 8; ++i) add((int)(rng() % (unsigned)res) - res / 4, (int)(rng() % (unsigned)res) - res / 4, (int)(rng() % (unsigned)res) - res / 4, res / 2, res / 3, res / 2);
  add(0, 0, 0, res, res, res);
  add(-5, -5, -5, res + 10, res + 10, res + 10);
  const size_t n = boxes.size() / 6;
  std::vector<uint8_t> ref(n), strict(n);
  if (!pipeline.collidesWith(boxes.data(), n, test, SE_HIP_COLLIDE_REFERENCE, ref.data())) { std::fprintf(stderr, "collidesWith failed\n"); return 4; }
  if (!pipeline.collidesWith(boxes.data(), n, test, SE_HIP_COLLIDE_STRICT, strict.data())) { std::fprintf(stderr, "collidesWith failed\n"); return 4; }
  // (for the record: what a host user pays -- getMap() once, then the single-threaded traversal per box)
  const auto t_cpu = std::chrono::steady_clock::now();
  long sink = 0;
  for (size_t i = 0; i < n; ++i) {
    const int32_t* b = &boxes[6 * i];
    sink += (long)se::geometry::collides_with(*map, se::geometry::int3{{b[0], b[1], b[2]}}, se::geometry::int3{{b[3], b[4], b[5]}}, host_test);
  }
  const double cpu_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_cpu).count();
  std::fprintf(stderr, "getmap_ms %.3f host_collides_us_per_box %.3f (sum %ld)\n", getmap_ms, cpu_us / (double)n, sink);
  long cnt[3] = {0, 0, 0}, differ = 0, bad = 0;
  for (size_t i = 0; i < n; ++i) {
    const int32_t* b = &boxes[6 * i];
    const se::geometry::int3 lo = {{b[0], b[1], b[2]}}, sd = {{b[3], b[4], b[5]}};
    const int r = (int)se::geometry::collides_with(*map, lo, sd, host_test);
    // strict by brute force: min over [lo, lo + side) of the class of Octree::get, outside the volume unseen
    int st = 2;
    for (int z = b[2]; z < b[2] + b[5] && st > 0; ++z)
      for (int y = b[1]; y < b[1] + b[4] && st > 0; ++y)
        for (int x = b[0]; x < b[0] + b[3] && st > 0; ++x) {
          const bool in = x >= 0 && y >= 0 && z >= 0 && x < res && y < res && z < res;
          const int c = in ? (int)host_test(map->get(x, y, z)) : 1;
          if (c < st) st = c;
        }
    if (r != (int)ref[i] || st != (int)strict[i]) {
      if (bad < 5) std::fprintf(stderr, "box %zu (%d %d %d | %d %d %d): reference %d device %d, strict %d device %d\n", i, b[0], b[1], b[2], b[3], b[4], b[5], r, ref[i], st, strict[i]);
      ++bad;
    }
    ++cnt[r];
    differ += r != st;
  }
  std::printf("checked %zu occupied %ld unseen %ld empty %ld differ %ld bad %ld\n", n, cnt[0], cnt[1], cnt[2], differ, bad);
  return 0;
}
