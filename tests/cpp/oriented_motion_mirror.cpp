// DenseSLAMSystem::collidesOrientedMoving (se_hip_collide_oriented_motions_host) against the host se::Octree that getMap() builds from the
// same device map: motion for motion with se::geometry::oriented_motion_status (include/se/oriented_motion.hpp), for both stop_at, on status,
// the reduced t_exact pair and the bits of t_first; a sample of small motions also against the literal brute-force definition.
//   usage: oriented_motion_mirror <scene.raw> <poses.bin> <volume_res> <volume_dim> <mu>
// Prints one line: "checked <n> occupied <n> unseen <n> empty <n> invalid <n> blocked <n> free <n> brute <n> rounded <n> rotated <n> bad <n>"
// (counts of the host answers with stop_at occupied; blocked = 0 < t_exact < 1; brute = motions also held to the definition; rotated = motions
// made by orientedMotion, rounded = those of them that equal se::geometry::oriented_motion_round's).
#include "mirror_scene.hpp"
#include <se/oriented_motion.hpp>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
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
  const int sub = SE_HIP_ORIENTED_SUB;
  std::mt19937 rng(37);
  std::uniform_real_distribution<double> uni(0.0, 1.0);
  std::normal_distribution<double> normal(0.0, 1.0);
  std::vector<int32_t> motions;
  long rounded = 0;
  // a box of the given half lengths (voxels) at a random attitude about the centre (voxels), moved by up to `reach` voxels in a random
  // direction, through the mirror's rounding helper
  auto add_rotated = [&](double cx, double cy, double cz, double l0, double l1, double l2, double reach, int kind) {
    double q[4], nrm = 0;
    for (int a = 0; a < 4; ++a) { q[a] = normal(rng); nrm += q[a] * q[a]; }
    nrm = std::sqrt(nrm);
    const double w = q[0] / nrm, x = q[1] / nrm, y = q[2] / nrm, z = q[3] / nrm;
    const double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)},
                            {2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)},
                            {2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
    const float vox = scene.dim / res;
    Eigen::Matrix4f pose = Eigen::Matrix4f::Identity();
    float rot[9];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) { pose(r, c) = (float)R[r][c]; rot[3 * r + c] = (float)R[r][c]; }
    const float centre[3] = {(float)cx * vox, (float)cy * vox, (float)cz * vox}, half[3] = {(float)l0 * vox, (float)l1 * vox, (float)l2 * vox};
    for (int k = 0; k < 3; ++k) pose(k, 3) = centre[k];
    double u[3], un = 0;
    for (int a = 0; a < 3; ++a) { u[a] = normal(rng); un += u[a] * u[a]; }
    const double step = uni(rng) * reach / std::sqrt(un);
    const float move[3] = {(float)(u[0] * step) * vox, (float)(u[1] * step) * vox, (float)(u[2] * step) * vox};
    int32_t m[15];
    pipeline.orientedMotion(pose, Eigen::Vector3f(half[0], half[1], half[2]), Eigen::Vector3f(move[0], move[1], move[2]), m);
    const se::geometry::oriented_motion same = se::geometry::oriented_motion_round(centre, rot, half, move, scene.dim, res);
    bool eq = true;
    for (int k = 0; k < 3; ++k) eq = eq && m[k] == same.box.c[k] && m[12 + k] == same.d[k];
    for (int i = 0; i < 3; ++i)
      for (int k = 0; k < 3; ++k) eq = eq && m[3 + 3 * i + k] == same.box.h[i][k];
    rounded += eq;
    if (kind == 1)   // skew
      for (int k = 0; k < 3; ++k) m[6 + k] += m[3 + k] / 2;
    if (kind == 2) m[12 + (int)(rng() % 3)] = 0;                       // a zero component
    if (kind == 3) m[12] = m[13] = m[14] = 0;                          // no motion
    if (kind == 4) for (int k = 0; k < 3; ++k) m[12 + k] = 2 * m[3 + k];   // along a half-axis
    motions.insert(motions.end(), m, m + 15);
  };
  auto len = [&](double hi) { return std::exp(uni(rng) * std::log(hi * sub)) / sub; };   // 1 / 16 voxel .. hi voxels
  // uniform (some partly or wholly outside), then around allocated blocks, where the surfaces are
  for (int i = 0; i < 300; ++i)
    add_rotated(uni(rng) * (res + 32) - 16, uni(rng) * (res + 32) - 16, uni(rng) * (res + 32) - 16, len(6), len(6), len(6), 24, i % 8);
  const auto& blocks = map->getBlockBuffer();
  const size_t n_small = 300;   // of the next set, these are small enough for the brute force
  for (int i = 0; i < 1200; ++i) {
    const int* c = blocks[rng() % blocks.size()]->coordinates();
    const double hi = (size_t)i < n_small ? 2 : 6;
    add_rotated(c[0] + uni(rng) * 24 - 8, c[1] + uni(rng) * 24 - 8, c[2] + uni(rng) * 24 - 8, len(hi), len(hi), len(hi), (size_t)i < n_small ? 8 : 24, i % 8);
  }
  const size_t n_rotated = motions.size() / 15;
  auto add = [&](std::initializer_list<int32_t> v) { motions.insert(motions.end(), v.begin(), v.end()); };
  for (int i = 0; i < 100; ++i) {   // axis-aligned on voxel boundaries, about allocated blocks, moved by whole voxels
    const int* c = blocks[rng() % blocks.size()]->coordinates();
    const int s[3] = {1 + (int)(rng() % 6), 1 + (int)(rng() % 6), 1 + (int)(rng() % 6)};
    add({sub * (c[0] + (int)(rng() % 12) - 2) + 8 * s[0], sub * (c[1] + (int)(rng() % 12) - 2) + 8 * s[1], sub * (c[2] + (int)(rng() % 12) - 2) + 8 * s[2],
         8 * s[0], 0, 0, 0, 8 * s[1], 0, 0, 0, 8 * s[2], sub * ((int)(rng() % 21) - 10), sub * ((int)(rng() % 21) - 10), sub * ((int)(rng() % 21) - 10)});
  }
  add({sub * res / 2, sub * res / 2, sub * res / 2, 8, 0, 0, 0, 8, 0, 0, 0, 8, sub * res, 0, 0});             // out through the x face
  add({-40 * sub, -40 * sub, -40 * sub, 30, 40, 0, -40, 30, 0, 0, 0, 50, 10, 20, 30});                         // wholly outside
  add({-4 * sub, sub * res / 2, sub * res / 2, 30, 40, 0, -40, 30, 0, 0, 0, 50, 2 * sub * res, 5, -7});        // across the whole volume
  add({100, 100, 100, 8, 8, 0, 1, 0, 0, 8, 8, 0, 16, 0, 0});                                                   // invalid: det = 0
  add({100, 100, 100, 8, 0, 0, 0, 8, 0, 0, 0, 8, (1 << 18) + 1, 0, 0});                                        // invalid: displacement beyond the limit
  add({(1 << 20) - 4, 0, 0, 8, 0, 0, 0, 8, 0, 0, 0, 8, 5, 0, 0});                                              // invalid: end beyond the limit
  const size_t n = motions.size() / 15;

  long cnt[4] = {0, 0, 0, 0}, blocked = 0, free_ = 0, brute = 0, bad = 0;
  for (int s = 0; s < 2; ++s) {
    const int32_t stop = s == 0 ? SE_HIP_COLLISION_OCCUPIED : SE_HIP_COLLISION_UNSEEN;
    const se::geometry::collision_status host_stop = s == 0 ? se::geometry::collision_status::occupied : se::geometry::collision_status::unseen;
    std::vector<uint8_t> status(n), status_alone(n);
    std::vector<float> t_first(n);
    std::vector<int64_t> t_exact(2 * n);
    se_hip_oriented_motion_out out = {status.data(), t_first.data(), t_exact.data()};
    se_hip_oriented_motion_out alone = {status_alone.data(), nullptr, nullptr};
    if (!pipeline.collidesOrientedMoving(motions.data(), n, test, stop, out) || !pipeline.collidesOrientedMoving(motions.data(), n, test, stop, alone)) {
      std::fprintf(stderr, "collidesOrientedMoving failed\n");
      return 4;
    }
    for (size_t i = 0; i < n; ++i) {
      const se::geometry::oriented_motion mo = se::geometry::oriented_motion_from(&motions[15 * i]);
      const se::geometry::oriented_motion_result r = se::geometry::oriented_motion_status(*map, mo, host_test, host_stop);
      const int st = r.valid ? (int)r.status : SE_HIP_COLLISION_INVALID;
      const float tf = se::geometry::oriented_motion_float(r.t_exact);
      bool same = st == (int)status[i] && st == (int)status_alone[i] && r.t_exact.num == t_exact[2 * i] && r.t_exact.den == t_exact[2 * i + 1] &&
                  std::memcmp(&tf, &t_first[i], sizeof(float)) == 0;
      if (i >= 300 && i < 300 + n_small) {
        const se::geometry::oriented_motion_result q = se::geometry::oriented_motion_status_brute(*map, mo, host_test, host_stop);
        same = same && q.valid == r.valid && (!q.valid || (q.status == r.status && q.t_exact.num == r.t_exact.num && q.t_exact.den == r.t_exact.den));
        brute += s == 0;
      }
      if (!same) {
        if (bad < 5) {
          std::fprintf(stderr, "stop %d motion %zu (", (int)stop, i);
          for (int k = 0; k < 15; ++k) std::fprintf(stderr, "%d ", motions[15 * i + k]);
          std::fprintf(stderr, "): host %d %lld / %lld, device %d (alone %d) %lld / %lld %g\n", st, (long long)r.t_exact.num, (long long)r.t_exact.den, (int)status[i],
                       (int)status_alone[i], (long long)t_exact[2 * i], (long long)t_exact[2 * i + 1], (double)t_first[i]);
        }
        ++bad;
      }
      if (s == 0) {
        ++cnt[r.valid ? st : 3];
        blocked += r.valid && r.t_exact.num > 0 && r.t_exact.num < r.t_exact.den;
        free_ += r.valid && r.t_exact.num == 2;
      }
    }
  }
  std::printf("checked %zu occupied %ld unseen %ld empty %ld invalid %ld blocked %ld free %ld brute %ld rounded %ld rotated %zu bad %ld\n", n, cnt[0], cnt[1], cnt[2], cnt[3],
              blocked, free_, brute, rounded, n_rotated, bad);
  return 0;
}
