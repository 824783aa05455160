// DenseSLAMSystem::reachField (se_hip_reach_field_host) against the host se::Octree that getMap() builds from the same device map: position
// for position with the literal definition se::geometry::reach_field (include/se/reach_field.hpp), steps, seed, next and the counts, for both
// stop_at values.
//   usage: reach_mirror <scene.raw> <poses.bin> <volume_res> <volume_dim> <mu>
// Prints one line: "requests <n> positions <n> blocked <n> reached <n> cut <n> outside <n> late <n> bad <n>" (counts over the positions of the
// host answers: not free, reached, free yet cut off from every seed; reached positions outside the volume; calls whose rounds exceed
// max steps + 2; positions or counts that differ).
#include "mirror_scene.hpp"
#include <se/reach_field.hpp>

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
  std::mt19937 rng(41);
  std::vector<se::geometry::reach_request> requests;
  // seeds: the region's corners first (free wherever the region's rim is), then random positions in and just around it
  auto add = [&](int x, int y, int z, int sx, int sy, int sz, int rx, int ry, int rz, int n_seeds) {
    se::geometry::reach_request q;
    q.lo = {{x, y, z}}; q.side = {{sx, sy, sz}}; q.robot = {{rx, ry, rz}};
    q.seeds.push_back({{x, y, z}});
    q.seeds.push_back({{x + sx - 1, y + sy - 1, z + sz - 1}});
    for (int s = 2; s < n_seeds; ++s) q.seeds.push_back({{x - 1 + (int)(rng() % (unsigned)(sx + 2)), y - 1 + (int)(rng() % (unsigned)(sy + 2)), z - 1 + (int)(rng() % (unsigned)(sz + 2))}});
    requests.push_back(q);
  };
  auto upto = [&](int hi) { return 1 + (int)(rng() % (unsigned)hi); };
  // around allocated blocks, where the surfaces are; then across a face of the volume, beyond it, and one with a robot as large as a block
  const auto& blocks = map->getBlockBuffer();
  for (int i = 0; i < 24; ++i) {
    const int* c = blocks[rng() % blocks.size()]->coordinates();
    add(c[0] + (int)(rng() % 16) - 8, c[1] + (int)(rng() % 16) - 8, c[2] + (int)(rng() % 16) - 8, 8 + upto(40), 4 + upto(16), 4 + upto(16), upto(3), upto(3), upto(3), upto(6));
  }
  add(-4, 10, 10, 40, 12, 9, 1, 1, 1, 3);
  add(res - 20, res - 9, 20, 36, 17, 10, 2, 2, 2, 4);
  add(res + 10, 5, 5, 3, 3, 3, 1, 1, 1, 2);
  {
    const int* c = blocks[rng() % blocks.size()]->coordinates();
    add(c[0] - 16, c[1] - 16, c[2] - 16, 34, 20, 20, 8, 8, 8, 4);
  }

  long positions = 0, kinds[3] = {0, 0, 0}, outside = 0, late = 0, bad = 0;
  for (int s = 0; s < 2; ++s) {
    const int32_t stop = s ? SE_HIP_COLLISION_UNSEEN : SE_HIP_COLLISION_OCCUPIED;
    const se::geometry::collision_status host_stop = s ? se::geometry::collision_status::unseen : se::geometry::collision_status::occupied;
    for (size_t n = 0; n < requests.size(); ++n) {
      const se::geometry::reach_request& q = requests[n];
      std::vector<int32_t> seeds;
      for (const se::geometry::int3& p : q.seeds)
        for (int k = 0; k < 3; ++k) seeds.push_back(p(k));
      se_hip_reach_request rq;
      for (int k = 0; k < 3; ++k) { rq.lo[k] = q.lo(k); rq.side[k] = q.side(k); rq.robot[k] = q.robot(k); }
      rq.stop_at = stop; rq.n_seeds = (int32_t)q.seeds.size(); rq.seeds = seeds.data();
      const size_t count = (size_t)q.side(0) * q.side(1) * q.side(2);
      std::vector<int32_t> steps(count), steps_only(count);
      std::vector<uint8_t> seed(count), next(count);
      int64_t counts[4] = {0, 0, 0, 0};
      se_hip_reach_out out = {steps.data(), seed.data(), next.data(), counts}, out1 = {steps_only.data(), nullptr, nullptr, nullptr};
      if (!pipeline.reachField(rq, test, out) || !pipeline.reachField(rq, test, out1)) { std::fprintf(stderr, "reachField failed\n"); return 4; }
      se::geometry::reach_result host;
      if (!se::geometry::reach_field(*map, q, host_test, host_stop, host)) { std::fprintf(stderr, "invalid request %zu\n", n); return 5; }
      if (counts[0] != host.counts[0] || counts[1] != host.counts[1] || counts[2] != host.counts[2]) {
        if (bad < 5)
          std::fprintf(stderr, "request %zu stop_at %d: counts host %ld %ld %ld, device %ld %ld %ld\n", n, (int)stop, (long)host.counts[0], (long)host.counts[1],
                       (long)host.counts[2], (long)counts[0], (long)counts[1], (long)counts[2]);
        ++bad;
      }
      if (counts[3] < 1 || counts[3] > host.counts[2] + 2) ++late;
      size_t i = 0;
      for (int z = 0; z < q.side(2); ++z)
        for (int y = 0; y < q.side(1); ++y)
          for (int x = 0; x < q.side(0); ++x, ++i) {
            const bool same = host.steps[i] == steps[i] && host.steps[i] == steps_only[i] && host.seed[i] == seed[i] && host.next[i] == next[i];
            if (!same) {
              if (bad < 5)
                std::fprintf(stderr, "request %zu position %zu stop_at %d: host %d %d %d, device %d %d %d (steps alone %d)\n", n, i, (int)stop, (int)host.steps[i],
                             (int)host.seed[i], (int)host.next[i], (int)steps[i], (int)seed[i], (int)next[i], (int)steps_only[i]);
              ++bad;
            }
            ++positions;
            if (host.steps[i] >= 0) {
              ++kinds[1];
              const int v[3] = {q.lo(0) + x, q.lo(1) + y, q.lo(2) + z};
              for (int k = 0; k < 3; ++k)
                if (v[k] < 0 || v[k] >= res) { ++outside; break; }
            }
          }
      kinds[0] += (long)count - (long)host.counts[0];
      kinds[2] += (long)(host.counts[0] - host.counts[1]);
    }
  }
  std::printf("requests %zu positions %ld blocked %ld reached %ld cut %ld outside %ld late %ld bad %ld\n", requests.size(), positions, kinds[0], kinds[1], kinds[2], outside,
              late, bad);
  return 0;
}
