// DenseSLAMSystem::clearanceOf (se_hip_clearance_boxes_host) against the host se::Octree that getMap() builds from the same device map:
// query for query with se::geometry::clearance (include/se/clearance.hpp), d2 and the nearest voxel, for both stop_at values; a sample of
// queries with a small r_max also against the literal brute-force definition.
//   usage: clearance_mirror <scene.raw> <poses.bin> <volume_res> <volume_dim> <mu>
// Prints one line: "checked <n> touching <n> apart <n> none <n> outside <n> brute <n> bad <n>" (counts of the host answers: with stop_at
// occupied d2 == 0, d2 > 0, nothing within r_max; with stop_at unseen a nearest voxel outside the volume; brute = queries also held to the
// definition).
#include "mirror_scene.hpp"
#include <se/clearance.hpp>

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
  pipeline.getMap(map);
  if (map->getBlockBuffer().empty()) { std::fprintf(stderr, "empty map\n"); return 3; }

  const bool ofusion = std::is_same<FieldType, OFusion>::value;
  const se_hip_collide_test test = {0.f, ofusion ? 1 : 0};
  const se::geometry::voxel_test<FieldType> host_test = {0.f, ofusion};
  std::mt19937 rng(31);
  std::vector<int32_t> queries;
  auto add = [&](int x, int y, int z, int a, int b, int c, int r) {
    const int32_t v[7] = {x, y, z, a, b, c, r};
    queries.insert(queries.end(), v, v + 7);
  };
  auto side = [&](int hi) { return 1 + (int)(rng() % (unsigned)hi); };
  // uniform (some outside), then around allocated blocks, where the surfaces are
  for (int i = 0; i < 200; ++i)
    add((int)(rng() % (unsigned)(res + 32)) - 16, (int)(rng() % (unsigned)(res + 32)) - 16, (int)(rng() % (unsigned)(res + 32)) - 16, side(10), side(10), side(10),
        (int)(rng() % 24));
  const auto& blocks = map->getBlockBuffer();
  const size_t n_brute = 200;   // of the next set, these have an r_max small enough for the brute force
  for (int i = 0; i < 500; ++i) {
    const int* c = blocks[rng() % blocks.size()]->coordinates();
    add(c[0] + (int)(rng() % 48) - 24, c[1] + (int)(rng() % 48) - 24, c[2] + (int)(rng() % 48) - 24, side(8), side(8), side(8),
        (size_t)i < n_brute ? (int)(rng() % 13) : (int)(rng() % 40));
  }
  add(0, 0, 0, res, res, res, 0);
  add(-40, -40, -40, 3, 3, 3, 60);
  add(res / 2, res / 2, res / 2, 1, 1, 1, 32767);
  add(0, 0, 0, 0, 1, 1, 4);                     // invalid: side 0
  add(1 << 19, 0, 0, 1, 1, 1, 4);               // invalid: lo + side beyond the limit
  add(0, 0, 0, 1, 1, 1, 32768);                 // invalid: r_max
  const size_t n = queries.size() / 7;

  long kinds[3] = {0, 0, 0}, outside = 0, brute = 0, bad = 0;
  for (int s = 0; s < 2; ++s) {
    const int32_t stop = s ? SE_HIP_COLLISION_UNSEEN : SE_HIP_COLLISION_OCCUPIED;
    const se::geometry::collision_status host_stop = s ? se::geometry::collision_status::unseen : se::geometry::collision_status::occupied;
    std::vector<int32_t> d2(n), d2_only(n), nearest(3 * n);
    se_hip_clearance_out out = {d2.data(), nearest.data()};
    if (!pipeline.clearanceOf(queries.data(), n, test, stop, out)) { std::fprintf(stderr, "clearanceOf failed\n"); return 4; }
    se_hip_clearance_out out1 = {d2_only.data(), nullptr};
    if (!pipeline.clearanceOf(queries.data(), n, test, stop, out1)) { std::fprintf(stderr, "clearanceOf failed\n"); return 4; }
    for (size_t i = 0; i < n; ++i) {
      const int32_t* b = &queries[7 * i];
      const se::geometry::int3 lo = {{b[0], b[1], b[2]}}, sd = {{b[3], b[4], b[5]}};
      const se::geometry::clearance_result r = se::geometry::clearance(*map, lo, sd, b[6], host_test, host_stop);
      bool same = r.d2 == (int64_t)d2[i] && r.d2 == (int64_t)d2_only[i] && r.nearest(0) == nearest[3 * i] && r.nearest(1) == nearest[3 * i + 1] &&
                  r.nearest(2) == nearest[3 * i + 2];
      if (i >= 200 && i < 200 + n_brute) {
        const se::geometry::clearance_result q = se::geometry::clearance_brute(*map, lo, sd, b[6], host_test, host_stop);
        same = same && q.d2 == r.d2 && q.nearest(0) == r.nearest(0) && q.nearest(1) == r.nearest(1) && q.nearest(2) == r.nearest(2);
        brute += s == 0;
      }
      if (!same) {
        if (bad < 5)
          std::fprintf(stderr, "query %zu (%d %d %d | %d %d %d | %d) stop_at %d: host %lld (%d %d %d), device %d (%d %d %d) (d2 alone %d)\n", i, b[0], b[1], b[2], b[3],
                       b[4], b[5], b[6], (int)stop, (long long)r.d2, r.nearest(0), r.nearest(1), r.nearest(2), (int)d2[i], (int)nearest[3 * i], (int)nearest[3 * i + 1],
                       (int)nearest[3 * i + 2], (int)d2_only[i]);
        ++bad;
      }
      if (s == 0 && r.d2 != se::geometry::clearance_invalid) ++kinds[r.d2 == 0 ? 0 : (r.d2 > 0 ? 1 : 2)];
      if (s == 1 && r.d2 >= 0)
        for (int k = 0; k < 3; ++k)
          if (r.nearest(k) < 0 || r.nearest(k) >= res) { ++outside; break; }
    }
  }
  std::printf("checked %zu touching %ld apart %ld none %ld outside %ld brute %ld bad %ld\n", n, kinds[0], kinds[1], kinds[2], outside, brute, bad);
  return 0;
}
