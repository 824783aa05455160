// DenseSLAMSystem::collidesMoving (se_hip_collide_motions_host) against the host se::Octree that getMap() builds from the same device map:
// motion for motion with se::geometry::motion_status_and_entry (include/se/motion_collision.hpp), status and the bits of t_first, for both
// stop_at values; a sample of short motions also against the literal brute-force definition.
//   usage: motion_mirror <scene.raw> <poses.bin> <volume_res> <volume_dim> <mu>
// Prints one line: "checked <n> occupied <n> unseen <n> empty <n> start <n> partial <n> free <n> brute <n> bad <n>" (counts of the host
// answers with stop_at occupied: statuses, then t_first == 0, strictly between 0 and 1, free; brute = motions also held to the definition).
#include "mirror_scene.hpp"
#include <se/motion_collision.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
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
  std::mt19937 rng(29);
  std::vector<int32_t> motions;
  auto add = [&](int x, int y, int z, int a, int b, int c, int dx, int dy, int dz) {
    const int32_t v[9] = {x, y, z, a, b, c, dx, dy, dz};
    motions.insert(motions.end(), v, v + 9);
  };
  auto side = [&](int hi) { return 1 + (int)(rng() % (unsigned)hi); };
  auto move = [&](int m) { return (int)(rng() % (unsigned)(2 * m + 1)) - m; };
  // uniform (some start or end outside), then around allocated blocks, where the surfaces are
  for (int i = 0; i < 500; ++i)
    add((int)(rng() % (unsigned)(res + 32)) - 16, (int)(rng() % (unsigned)(res + 32)) - 16, (int)(rng() % (unsigned)(res + 32)) - 16, side(10), side(10), side(10),
        move(48), move(48), move(48));
  const auto& blocks = map->getBlockBuffer();
  const size_t n_short = 300;   // of the next set, these are short enough for the brute force
  for (int i = 0; i < 1300; ++i) {
    const int* c = blocks[rng() % blocks.size()]->coordinates();
    const int m = (size_t)i < n_short ? 12 : 40;
    add(c[0] + (int)(rng() % 40) - 20, c[1] + (int)(rng() % 40) - 20, c[2] + (int)(rng() % 40) - 20, side(8), side(8), side(8),
        i % 7 == 0 ? 0 : move(m), i % 5 == 0 ? 0 : move(m), i % 3 == 0 ? 0 : move(m));
  }
  add(0, 0, 0, 4, 4, 4, res - 4, res - 4, res - 4);
  add(res - 4, 0, res - 4, 4, 4, 4, -(res - 4), res - 4, -(res - 4));
  add(-40, -40, -40, 3, 3, 3, 10, 0, 5);
  add(0, 0, 0, 0, 1, 1, 1, 1, 1);                     // invalid: side 0
  add(1 << 20, 0, 0, 1, 1, 1, 0, 0, 0);               // invalid: lo + side beyond the limit
  const size_t n = motions.size() / 9;

  long cnt[3] = {0, 0, 0}, kinds[3] = {0, 0, 0}, brute = 0, bad = 0;
  for (int s = 0; s < 2; ++s) {
    const int32_t stop = s ? SE_HIP_COLLISION_UNSEEN : SE_HIP_COLLISION_OCCUPIED;
    const se::geometry::collision_status host_stop = s ? se::geometry::collision_status::unseen : se::geometry::collision_status::occupied;
    std::vector<uint8_t> status(n), status_only(n);
    std::vector<float> t_first(n);
    se_hip_motion_out out = {status.data(), t_first.data()};
    if (!pipeline.collidesMoving(motions.data(), n, test, stop, out)) { std::fprintf(stderr, "collidesMoving failed\n"); return 4; }
    se_hip_motion_out out1 = {status_only.data(), nullptr};
    if (!pipeline.collidesMoving(motions.data(), n, test, stop, out1)) { std::fprintf(stderr, "collidesMoving failed\n"); return 4; }
    for (size_t i = 0; i < n; ++i) {
      const int32_t* b = &motions[9 * i];
      const se::geometry::int3 lo = {{b[0], b[1], b[2]}}, sd = {{b[3], b[4], b[5]}}, d = {{b[6], b[7], b[8]}};
      const se::geometry::motion_result r = se::geometry::motion_status_and_entry(*map, lo, sd, d, host_test, host_stop);
      const int st = r.valid ? (int)r.status : SE_HIP_COLLISION_INVALID;
      const float t = se::geometry::to_float(r.t_first);
      bool same = st == (int)status[i] && st == (int)status_only[i] && std::memcmp(&t, &t_first[i], 4) == 0;
      if (i >= 500 && i < 500 + n_short) {
        const se::geometry::motion_result q = se::geometry::motion_status_and_entry_brute(*map, lo, sd, d, host_test, host_stop);
        same = same && q.status == r.status && q.t_first.num == r.t_first.num && q.t_first.den == r.t_first.den;
        brute += s == 0;
      }
      if (!same) {
        if (bad < 5)
          std::fprintf(stderr, "motion %zu (%d %d %d | %d %d %d | %d %d %d) stop_at %d: host %d %g, device %d %g (status alone %d)\n", i, b[0], b[1], b[2], b[3], b[4], b[5],
                       b[6], b[7], b[8], (int)stop, st, (double)t, (int)status[i], (double)t_first[i], (int)status_only[i]);
        ++bad;
      }
      if (s == 0 && r.valid) {
        ++cnt[st];
        ++kinds[t == 0.f ? 0 : (t < 1.f ? 1 : 2)];
      }
    }
  }
  std::printf("checked %zu occupied %ld unseen %ld empty %ld start %ld partial %ld free %ld brute %ld bad %ld\n", n, cnt[0], cnt[1], cnt[2], kinds[0], kinds[1], kinds[2],
              brute, bad);
  return 0;
}
