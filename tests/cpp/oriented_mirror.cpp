// DenseSLAMSystem::collidesOriented (se_hip_collide_oriented_host) against the host se::Octree that getMap() builds from the same device map:
// box for box with se::geometry::oriented_status (include/se/oriented_collision.hpp); a sample of small boxes also against the literal
// brute-force definition.
//   usage: oriented_mirror <scene.raw> <poses.bin> <volume_res> <volume_dim> <mu>
// Prints one line: "checked <n> occupied <n> unseen <n> empty <n> invalid <n> brute <n> rounded <n> rotated <n> bad <n>" (counts of the host
// answers; brute = boxes also held to the definition; rotated = boxes made by orientedBox, rounded = those of them that equal
// se::geometry::oriented_box_round's).
#include "mirror_scene.hpp"
#include <se/oriented_collision.hpp>

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
  std::mt19937 rng(31);
  std::uniform_real_distribution<double> uni(0.0, 1.0);
  std::normal_distribution<double> normal(0.0, 1.0);
  std::vector<int32_t> boxes;
  long rounded = 0;
  // a box of the given half lengths (voxels) at a random attitude about the centre (voxels), through the mirror's rounding helper
  auto add_rotated = [&](double cx, double cy, double cz, double l0, double l1, double l2, bool skew) {
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
    int32_t b[12];
    pipeline.orientedBox(pose, Eigen::Vector3f(half[0], half[1], half[2]), b);
    const se::geometry::oriented_box same = se::geometry::oriented_box_round(centre, rot, half, scene.dim, res);
    bool eq = true;
    for (int k = 0; k < 3; ++k) eq = eq && b[k] == same.c[k];
    for (int i = 0; i < 3; ++i)
      for (int k = 0; k < 3; ++k) eq = eq && b[3 + 3 * i + k] == same.h[i][k];
    rounded += eq;
    if (skew)
      for (int k = 0; k < 3; ++k) b[6 + k] += b[3 + k] / 2;
    boxes.insert(boxes.end(), b, b + 12);
  };
  auto len = [&](double hi) { return std::exp(uni(rng) * std::log(hi * sub)) / sub; };   // 1 / 16 voxel .. hi voxels
  // uniform (some partly or wholly outside), then around allocated blocks, where the surfaces are
  for (int i = 0; i < 500; ++i)
    add_rotated(uni(rng) * (res + 32) - 16, uni(rng) * (res + 32) - 16, uni(rng) * (res + 32) - 16, len(8), len(8), len(8), i % 5 == 0);
  const auto& blocks = map->getBlockBuffer();
  const size_t n_small = 400;   // of the next set, these are small enough for the brute force
  for (int i = 0; i < 1500; ++i) {
    const int* c = blocks[rng() % blocks.size()]->coordinates();
    const double hi = (size_t)i < n_small ? 3 : 8;
    add_rotated(c[0] + uni(rng) * 24 - 8, c[1] + uni(rng) * 24 - 8, c[2] + uni(rng) * 24 - 8, len(hi), len(hi), len(hi), i % 4 == 0);
  }
  const size_t n_rotated = boxes.size() / 12;
  auto add = [&](std::initializer_list<int32_t> v) { boxes.insert(boxes.end(), v.begin(), v.end()); };
  for (int i = 0; i < 100; ++i) {   // axis-aligned on voxel boundaries, about allocated blocks
    const int* c = blocks[rng() % blocks.size()]->coordinates();
    const int s[3] = {1 + (int)(rng() % 9), 1 + (int)(rng() % 9), 1 + (int)(rng() % 9)};
    add({sub * (c[0] + (int)(rng() % 12) - 2) + 8 * s[0], sub * (c[1] + (int)(rng() % 12) - 2) + 8 * s[1], sub * (c[2] + (int)(rng() % 12) - 2) + 8 * s[2],
         8 * s[0], 0, 0, 0, 8 * s[1], 0, 0, 0, 8 * s[2]});
  }
  add({sub * res / 2, sub * res / 2, sub * res / 2, 8 * res, 0, 0, 0, 8 * res, 0, 0, 0, 8 * res});        // exactly the volume
  add({sub * res / 2, sub * res / 2, sub * res / 2, 8 * res + 1, 0, 0, 0, 8 * res, 0, 0, 0, 8 * res});    // one sub-unit beyond it
  add({-40 * sub, -40 * sub, -40 * sub, 30, 40, 0, -40, 30, 0, 0, 0, 50});                                // wholly outside
  add({100, 100, 100, 8, 8, 0, 1, 0, 0, 8, 8, 0});                                                        // invalid: det = 0
  add({(1 << 20) + 1, 0, 0, 8, 0, 0, 0, 8, 0, 0, 0, 8});                                                  // invalid: centre beyond the limit
  add({0, 0, 0, (1 << 14) + 1, 0, 0, 0, 8, 0, 0, 0, 8});                                                  // invalid: half-axis beyond the limit
  const size_t n = boxes.size() / 12;

  std::vector<uint8_t> status(n);
  if (!pipeline.collidesOriented(boxes.data(), n, test, status.data())) { std::fprintf(stderr, "collidesOriented failed\n"); return 4; }
  long cnt[4] = {0, 0, 0, 0}, brute = 0, bad = 0;
  for (size_t i = 0; i < n; ++i) {
    const int32_t* b = &boxes[12 * i];
    const se::geometry::oriented_box box = se::geometry::oriented_box_from(b);
    const se::geometry::oriented_result r = se::geometry::oriented_status(*map, box, host_test);
    const int st = r.valid ? (int)r.status : SE_HIP_COLLISION_INVALID;
    bool same = st == (int)status[i];
    if (i >= 500 && i < 500 + n_small) {
      const se::geometry::oriented_result q = se::geometry::oriented_status_brute(*map, box, host_test);
      same = same && q.valid == r.valid && (!q.valid || q.status == r.status);
      ++brute;
    }
    if (!same) {
      if (bad < 5) {
        std::fprintf(stderr, "box %zu (", i);
        for (int k = 0; k < 12; ++k) std::fprintf(stderr, "%d ", b[k]);
        std::fprintf(stderr, "): host %d, device %d\n", st, (int)status[i]);
      }
      ++bad;
    }
    ++cnt[r.valid ? st : 3];
  }
  std::printf("checked %zu occupied %ld unseen %ld empty %ld invalid %ld brute %ld rounded %ld rotated %zu bad %ld\n", n, cnt[0], cnt[1], cnt[2], cnt[3], brute, rounded,
              n_rotated, bad);
  return 0;
}
