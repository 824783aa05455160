// DenseSLAMSystem::queryMap (se_hip_query_points_host) against the host se::Octree that getMap() builds from the same device map
// (include/se/octree.hpp): x and y of get_fine / get, interp and grad, bit for bit.  Drives the mirror over a SLAMBench .raw stream
// with ground-truth poses, the way examples/denseslam_raw.cpp does.
//   usage: map_query_mirror <scene.raw> <poses.bin> <volume_res> <volume_dim> <mu>
// Prints one line: "checked <n> in_volume <n> allocated <n> observed <n> coarse_node <n> bad <n>".
#include "mirror_scene.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

struct V3 {
  float v[3];
  float& operator()(int i) { return v[i]; }
  float operator()(int i) const { return v[i]; }
};

static bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

int main(int argc, char** argv) {
  MirrorScene scene;
  if (int rc = scene.replay(argc, argv, 6, "scene.raw poses.bin res dim mu")) return rc;
  DenseSLAMSystem& pipeline = *scene.pipeline;
  const int res = scene.res;
  const float dim = scene.dim;
  std::shared_ptr<se::Octree<FieldType> > map;
  pipeline.getMap(map);
  if (map->getBlockBuffer().empty()) { std::fprintf(stderr, "empty map\n"); return 3; }

  // points (voxel units first, metres = voxel / s): uniform in the volume, around allocated blocks (inside them, across their faces,
  // edges and corners, into the unallocated neighbours), and just outside each face of the volume
  const float s = (float)res / dim;
  std::mt19937 rng(17);
  std::uniform_real_distribution<float> U(0.f, 1.f);
  std::vector<float> pts;
  auto add = [&](float x, float y, float z) { pts.push_back(x / s); pts.push_back(y / s); pts.push_back(z / s); };
  for (int i = 0; i < 4000; ++i) add(U(rng) * res, U(rng) * res, U(rng) * res);
  const auto& blocks = map->getBlockBuffer();
  for (size_t i = 0; i < blocks.size(); i += 1 + blocks.size() / 1500) {
    const int* c = blocks[i]->coordinates();
    for (int j = 0; j < 3; ++j) add(c[0] - 4.f + 16.f * U(rng), c[1] - 4.f + 16.f * U(rng), c[2] - 4.f + 16.f * U(rng));
    add(c[0] + 7.5f, c[1] + 8.f * U(rng), c[2] + 8.f * U(rng));
    add(c[0] + 7.5f, c[1] + 7.5f, c[2] + 8.f * U(rng));
    add(c[0] + 7.5f, c[1] + 7.5f, c[2] + 7.5f);
    add(c[0] + 7.9f * U(rng), c[1] - 0.5f, c[2] + 7.9f * U(rng));
  }
  for (int face = 0; face < 6; ++face)
    for (int i = 0; i < 100; ++i) {
      float q[3] = {U(rng) * res, U(rng) * res, U(rng) * res};
      q[face / 2] = (face & 1) ? res + 1.5f * U(rng) : -1.5f * U(rng);
      add(q[0], q[1], q[2]);
    }
  const size_t n = pts.size() / 3;
  std::vector<float> fine(2 * n), coarse(2 * n), interp(n), grad(3 * n);
  std::vector<uint8_t> status(n);
  se_hip_query_out out{fine.data(), coarse.data(), interp.data(), grad.data(), status.data()};
  if (!pipeline.queryMap(pts.data(), n, out)) return 4;

  size_t in_volume = 0, allocated = 0, observed = 0, coarse_node = 0, bad = 0;
  auto sel = [](const se::Octree<FieldType>::value_type& v) { return v.x; };
  for (size_t i = 0; i < n; ++i) {
    V3 q;
    for (int a = 0; a < 3; ++a) q(a) = s * pts[3 * i + a];
    const int x = (int)q(0), y = (int)q(1), z = (int)q(2);
    const bool in = (unsigned)x < (unsigned)res && (unsigned)y < (unsigned)res && (unsigned)z < (unsigned)res;
    const auto f = map->get_fine(x, y, z);
    bool ok = same(fine[2 * i], f.x) && same(fine[2 * i + 1], (float)f.y);
    if (in) {   // (Octree::get walks unchecked bits: compared inside the volume, where it is defined)
      const auto c = map->get(x, y, z);
      ok = ok && same(coarse[2 * i], c.x) && same(coarse[2 * i + 1], (float)c.y);
      const bool alloc = map->fetch(x, y, z) != nullptr;
      if (!alloc && (!same(c.x, f.x) || (float)c.y != (float)f.y)) ++coarse_node;
      ok = ok && (((status[i] >> 1) & 1) == (alloc ? 1 : 0));
      allocated += alloc;
    }
    ok = ok && ((status[i] & 1) == (in ? 1 : 0));
    in_volume += in;
    observed += (status[i] >> 2) & 1;
    ok = ok && same(interp[i], map->interp(q, sel));
    const V3 g = map->grad(q);
    ok = ok && same(grad[3 * i], g(0)) && same(grad[3 * i + 1], g(1)) && same(grad[3 * i + 2], g(2));
    if (!ok && bad < 5)
      std::fprintf(stderr, "mismatch at q = (%.9g %.9g %.9g): fine %g/%g vs %g, interp %.9g vs %.9g, status %d\n", q(0), q(1), q(2), fine[2 * i],
                   fine[2 * i + 1], f.x, interp[i], map->interp(q, sel), status[i]);
    bad += !ok;
  }
  std::printf("checked %zu in_volume %zu allocated %zu observed %zu coarse_node %zu bad %zu\n", n, in_volume, allocated, observed, coarse_node, bad);
  return 0;
}
