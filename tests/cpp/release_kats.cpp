/*
 * Tests of se::release_map (include/se/release_map.hpp), the host restatement that defines the device's se_hip_release_boxes.
 *
 *   release_kats dump <sdf|ofusion> <in> <out>
 *     in:  int32 size, int32 k, se_hip_release_box records[k], uint64 nn, nn x {uint64 key, float x[8], float y[8]},
 *          uint64 nb, nb x {int32 corner[3], int32 active, float x[512], float y[512]}, uint64 nq, int32 points[nq][3]
 *     The tree is built from that (octants in any order), Octree::get is taken at the points, the k records are applied in ONE call, get is
 *     taken again, and the result is written:
 *     out: int64 accepted (0: the call refused the records), int64 counts[5], int32 touched[6], int64 bad (octants that fetch / fetch_octant
 *          do not find at their corner, keys out of order, wrong sides, children that are not in the buffers),
 *          uint64 nn, keys[nn], uint32 sides[nn], float x[nn][8], float y[nn][8],
 *          uint64 nb, keys[nb], int32 corners[nb][3], uint8 active[nb], float x[nb][512], float y[nb][512],
 *          float get_before[nq][2], float get_after[nq][2]
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "se/release_map.hpp"

template <typename T> static int run_dump(const char* in, const char* out) {
  FILE* f = std::fopen(in, "rb");
  if (!f) return 2;
  int32_t size = 0, k = 0;
  bool ok = std::fread(&size, 4, 1, f) == 1 && std::fread(&k, 4, 1, f) == 1 && k >= 0;
  std::vector<se_hip_release_box> recs((size_t)(ok ? k : 0));
  ok = ok && (recs.empty() || std::fread(recs.data(), sizeof(se_hip_release_box), recs.size(), f) == recs.size());
  int max_level = 0;
  for (int v = size; v > 1; v >>= 1) ++max_level;
  se::Octree<T> map;
  map.init(size, 5.f);
  uint64_t nn = 0, nb = 0, nq = 0;
  ok = ok && std::fread(&nn, 8, 1, f) == 1;
  for (uint64_t i = 0; i < nn && ok; ++i) {
    uint64_t key = 0; float x[8], y[8];
    ok = std::fread(&key, 8, 1, f) == 1 && std::fread(x, 4, 8, f) == 8 && std::fread(y, 4, 8, f) == 8;
    auto* n = map.add_node(key, (unsigned)(size >> (int)(key & 0x1FF)));
    for (int j = 0; j < 8; ++j) { n->value_[j].x = x[j]; n->value_[j].y = y[j]; }
  }
  ok = ok && std::fread(&nb, 8, 1, f) == 1;
  std::vector<float> x(512), y(512);
  for (uint64_t i = 0; i < nb && ok; ++i) {
    int32_t c[4];
    ok = std::fread(c, 4, 4, f) == 4 && std::fread(x.data(), 4, 512, f) == 512 && std::fread(y.data(), 4, 512, f) == 512;
    auto* b = map.add_block(se::alloc_detail::make_key(c[0], c[1], c[2], max_level - 3), c, c[3] != 0);
    for (int j = 0; j < 512; ++j) { b->voxel_block_[j].x = x[j]; b->voxel_block_[j].y = y[j]; }
  }
  ok = ok && std::fread(&nq, 8, 1, f) == 1;
  std::vector<int32_t> pts((size_t)(ok ? nq : 0) * 3);
  ok = ok && (pts.empty() || std::fread(pts.data(), 4, pts.size(), f) == pts.size());
  std::fclose(f);
  if (!ok) return 2;
  map.finalize();

  std::vector<float> got((size_t)nq * 4);
  auto sample = [&](size_t at) {
    for (uint64_t i = 0; i < nq; ++i) { const auto v = map.get(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]); got[at + 2 * i] = v.x; got[at + 2 * i + 1] = (float)v.y; }
  };
  sample(0);
  int64_t counts[5] = {77, 77, 77, 77, 77};
  int32_t touched[6] = {77, 77, 77, 77, 77, 77};
  const int64_t accepted = se::release_map(map, recs.data(), recs.size(), counts, touched) ? 1 : 0;
  sample((size_t)nq * 2);

  int64_t bad = 0;
  uint64_t prev = 0; bool first = true;
  std::set<const void*> live;
  for (auto& n : map.getNodesBuffer()) live.insert(n.get());
  for (auto& b : map.getBlockBuffer()) live.insert(b.get());
  for (auto& n : map.getNodesBuffer()) {
    const int level = (int)(n->code_ & 0x1FF);
    const uint64_t code = n->code_ & ~0x1FFull;
    const int c[3] = {se::release_detail::compact21(code, 0), se::release_detail::compact21(code, 1), se::release_detail::compact21(code, 2)};
    if (map.fetch_octant(c[0], c[1], c[2], level) != n.get() || (int)n->side_ != size >> level) ++bad;
    if (!first && n->code_ <= prev) ++bad;
    for (int j = 0; j < 8; ++j) {
      if ((n->child_ptr_[j] != nullptr) != (((n->children_mask_ >> j) & 1) != 0)) ++bad;
      if (n->child_ptr_[j] && !live.count(n->child_ptr_[j])) ++bad;
    }
    prev = n->code_; first = false;
  }
  first = true;
  for (auto& b : map.getBlockBuffer()) {
    const int* c = b->coordinates();
    if (map.fetch(c[0], c[1], c[2]) != b.get() || b->code_ != se::alloc_detail::make_key(c[0], c[1], c[2], max_level - 3)) ++bad;
    if (!first && b->code_ <= prev) ++bad;
    prev = b->code_; first = false;
  }
  if (map.root() == nullptr || map.root()->code_ != 0) ++bad;

  FILE* o = std::fopen(out, "wb");
  if (!o) return 2;
  std::fwrite(&accepted, 8, 1, o);
  std::fwrite(counts, 8, 5, o);
  std::fwrite(touched, 4, 6, o);
  std::fwrite(&bad, 8, 1, o);
  nn = map.getNodesBuffer().size();
  std::fwrite(&nn, 8, 1, o);
  for (auto& n : map.getNodesBuffer()) std::fwrite(&n->code_, 8, 1, o);
  for (auto& n : map.getNodesBuffer()) { const uint32_t s = n->side_; std::fwrite(&s, 4, 1, o); }
  for (auto& n : map.getNodesBuffer()) for (auto& v : n->value_) { const float t = v.x; std::fwrite(&t, 4, 1, o); }
  for (auto& n : map.getNodesBuffer()) for (auto& v : n->value_) { const float t = (float)v.y; std::fwrite(&t, 4, 1, o); }
  nb = map.getBlockBuffer().size();
  std::fwrite(&nb, 8, 1, o);
  for (auto& b : map.getBlockBuffer()) std::fwrite(&b->code_, 8, 1, o);
  for (auto& b : map.getBlockBuffer()) std::fwrite(b->coordinates_, 4, 3, o);
  for (auto& b : map.getBlockBuffer()) { const uint8_t a = b->active_ ? 1 : 0; std::fwrite(&a, 1, 1, o); }
  for (auto& b : map.getBlockBuffer()) for (auto& v : b->voxel_block_) { const float t = v.x; std::fwrite(&t, 4, 1, o); }
  for (auto& b : map.getBlockBuffer()) for (auto& v : b->voxel_block_) { const float t = (float)v.y; std::fwrite(&t, 4, 1, o); }
  if (!got.empty()) std::fwrite(got.data(), 4, got.size(), o);
  std::fclose(o);
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 5 && !std::strcmp(argv[1], "dump")) {
    if (!std::strcmp(argv[2], "sdf")) return run_dump<SDF>(argv[3], argv[4]);
    if (!std::strcmp(argv[2], "ofusion")) return run_dump<OFusion>(argv[3], argv[4]);
  }
  std::fprintf(stderr, "usage: %s dump <sdf|ofusion> <in.bin> <out.bin>\n", argv[0]);
  return 2;
}
