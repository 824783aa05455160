// DenseSLAMSystem::distanceField (se_hip_distance_field_host) against the host se::Octree that getMap() builds from the same device map:
// voxel for voxel with the literal definition se::geometry::distance_field_brute (include/se/distance_field.hpp), d2 and the nearest voxel,
// for both stop_at values.
//   usage: field_mirror <scene.raw> <poses.bin> <volume_res> <volume_dim> <mu>
// Prints one line: "requests <n> voxels <n> touching <n> apart <n> none <n> outside <n> bad <n>" (counts over the voxels of the host answers:
// with stop_at occupied d2 == 0, d2 > 0, nothing within r_max; with stop_at unseen a nearest voxel outside the volume).
#include "mirror_scene.hpp"
#include <se/distance_field.hpp>

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
  std::mt19937 rng(37);
  std::vector<se::geometry::field_request> requests;
  auto add = [&](int x, int y, int z, int sx, int sy, int sz, int rx, int ry, int rz, int r) {
    requests.push_back({{{x, y, z}}, {{sx, sy, sz}}, {{rx, ry, rz}}, r});
  };
  auto upto = [&](int hi) { return 1 + (int)(rng() % (unsigned)hi); };
  // around allocated blocks, where the surfaces are; then across a face of the volume, beyond it, and one with a robot as large as a block
  const auto& blocks = map->getBlockBuffer();
  for (int i = 0; i < 24; ++i) {
    const int* c = blocks[rng() % blocks.size()]->coordinates();
    add(c[0] + (int)(rng() % 16) - 8, c[1] + (int)(rng() % 16) - 8, c[2] + (int)(rng() % 16) - 8, upto(5), upto(5), upto(5), upto(3), upto(3), upto(3), (int)(rng() % 6));
  }
  add(-4, 10, 10, 9, 5, 3, 1, 1, 1, 5);
  add(res - 3, res - 3, 20, 6, 6, 4, 2, 2, 2, 4);
  add(res + 10, 5, 5, 3, 3, 3, 1, 1, 1, 6);
  {
    const int* c = blocks[rng() % blocks.size()]->coordinates();
    add(c[0] - 6, c[1] - 6, c[2] - 6, 4, 4, 4, 8, 8, 8, 3);
  }

  long voxels = 0, kinds[3] = {0, 0, 0}, outside = 0, bad = 0;
  for (int s = 0; s < 2; ++s) {
    const int32_t stop = s ? SE_HIP_COLLISION_UNSEEN : SE_HIP_COLLISION_OCCUPIED;
    const se::geometry::collision_status host_stop = s ? se::geometry::collision_status::unseen : se::geometry::collision_status::occupied;
    for (size_t n = 0; n < requests.size(); ++n) {
      const se::geometry::field_request& q = requests[n];
      se_hip_field_request rq;
      for (int k = 0; k < 3; ++k) { rq.lo[k] = q.lo(k); rq.side[k] = q.side(k); rq.robot[k] = q.robot(k); }
      rq.r_max = q.r_max; rq.stop_at = stop;
      const size_t count = (size_t)q.side(0) * q.side(1) * q.side(2);
      std::vector<int32_t> d2(count), d2_only(count), nearest(3 * count);
      se_hip_field_out out = {d2.data(), nearest.data()}, out1 = {d2_only.data(), nullptr};
      if (!pipeline.distanceField(rq, test, out) || !pipeline.distanceField(rq, test, out1)) { std::fprintf(stderr, "distanceField failed\n"); return 4; }
      se::geometry::field_result host;
      if (!se::geometry::distance_field_brute(*map, q, host_test, host_stop, host)) { std::fprintf(stderr, "invalid request %zu\n", n); return 5; }
      for (size_t i = 0; i < count; ++i) {
        const bool same = host.d2[i] == d2[i] && host.d2[i] == d2_only[i] && host.nearest[3 * i] == nearest[3 * i] && host.nearest[3 * i + 1] == nearest[3 * i + 1] &&
                          host.nearest[3 * i + 2] == nearest[3 * i + 2];
        if (!same) {
          if (bad < 5)
            std::fprintf(stderr, "request %zu voxel %zu stop_at %d: host %d (%d %d %d), device %d (%d %d %d) (d2 alone %d)\n", n, i, (int)stop, (int)host.d2[i],
                         (int)host.nearest[3 * i], (int)host.nearest[3 * i + 1], (int)host.nearest[3 * i + 2], (int)d2[i], (int)nearest[3 * i], (int)nearest[3 * i + 1],
                         (int)nearest[3 * i + 2], (int)d2_only[i]);
          ++bad;
        }
        if (s == 0) { ++voxels; ++kinds[host.d2[i] == 0 ? 0 : (host.d2[i] > 0 ? 1 : 2)]; }
        if (s == 1 && host.d2[i] >= 0)
          for (int k = 0; k < 3; ++k)
            if (host.nearest[3 * i + k] < 0 || host.nearest[3 * i + k] >= res) { ++outside; break; }
      }
    }
  }
  std::printf("requests %zu voxels %ld touching %ld apart %ld none %ld outside %ld bad %ld\n", requests.size(), voxels, kinds[0], kinds[1], kinds[2], outside, bad);
  return 0;
}
