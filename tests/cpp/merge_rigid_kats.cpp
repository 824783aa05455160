/*
 * Tests of se::merge_map_rigid / se::rigid_sample (include/se/merge_rigid.hpp), the host restatement that defines the device's
 * se_hip_merge_map_rigid.
 *
 *   merge_rigid_kats dump <sdf|ofusion> <in> <out>
 *     in:  int32 dst_size, int32 src_size, int32 mode, int32 same (1: src is dst itself), float max_weight, float src_dim_factor,
 *          float pull[12], then the destination tree and the source tree, each
 *            uint64 nn, nn x {uint64 key, float x[8], float y[8]}, uint64 nb, nb x {int32 corner[3], int32 active, float x[512], float y[512]}
 *     Both trees are built from that (octants in any order; dim = 0.0375 * size, the source's times src_dim_factor), the merge is applied,
 *     and the destination is written, then the source:
 *     out: int64 counts[10], int64 bad (octants that fetch / fetch_octant do not find at their corner, keys out of order, wrong sides),
 *          2 x {uint64 nn, keys[nn], uint32 sides[nn], float x[nn][8], float y[nn][8],
 *               uint64 nb, keys[nb], int32 corners[nb][3], uint8 active[nb], float x[nb][512], float y[nb][512]}
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "se/merge_rigid.hpp"

template <typename T> static bool read_tree(FILE* f, se::Octree<T>& map, int size, float dim) {
  int max_level = 0;
  for (int v = size; v > 1; v >>= 1) ++max_level;
  map.init(size, dim);
  uint64_t nn = 0, nb = 0;
  bool ok = std::fread(&nn, 8, 1, f) == 1;
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
  if (ok) map.finalize();
  return ok;
}

template <typename T> static int64_t check_tree(se::Octree<T>& map) {
  const int size = map.size();
  int max_level = 0;
  for (int v = size; v > 1; v >>= 1) ++max_level;
  int64_t bad = 0;
  uint64_t prev = 0; bool first = true;
  for (auto& n : map.getNodesBuffer()) {
    const int level = (int)(n->code_ & 0x1FF);
    const uint64_t code = n->code_ & ~0x1FFull;
    const int c[3] = {se::shift_detail::compact21(code, 0), se::shift_detail::compact21(code, 1), se::shift_detail::compact21(code, 2)};
    if (map.fetch_octant(c[0], c[1], c[2], level) != n.get() || (int)n->side_ != size >> level) ++bad;
    if (!first && n->code_ <= prev) ++bad;
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
  return bad;
}

template <typename T> static void write_tree(FILE* o, se::Octree<T>& map) {
  uint64_t nn = map.getNodesBuffer().size();
  std::fwrite(&nn, 8, 1, o);
  for (auto& n : map.getNodesBuffer()) std::fwrite(&n->code_, 8, 1, o);
  for (auto& n : map.getNodesBuffer()) { const uint32_t s = n->side_; std::fwrite(&s, 4, 1, o); }
  for (auto& n : map.getNodesBuffer()) for (auto& v : n->value_) { const float t = v.x; std::fwrite(&t, 4, 1, o); }
  for (auto& n : map.getNodesBuffer()) for (auto& v : n->value_) { const float t = (float)v.y; std::fwrite(&t, 4, 1, o); }
  uint64_t nb = map.getBlockBuffer().size();
  std::fwrite(&nb, 8, 1, o);
  for (auto& b : map.getBlockBuffer()) std::fwrite(&b->code_, 8, 1, o);
  for (auto& b : map.getBlockBuffer()) std::fwrite(b->coordinates_, 4, 3, o);
  for (auto& b : map.getBlockBuffer()) { const uint8_t a = b->active_ ? 1 : 0; std::fwrite(&a, 1, 1, o); }
  for (auto& b : map.getBlockBuffer()) for (auto& v : b->voxel_block_) { const float t = v.x; std::fwrite(&t, 4, 1, o); }
  for (auto& b : map.getBlockBuffer()) for (auto& v : b->voxel_block_) { const float t = (float)v.y; std::fwrite(&t, 4, 1, o); }
}

template <typename T> static int run_dump(const char* in, const char* out) {
  FILE* f = std::fopen(in, "rb");
  if (!f) return 2;
  int32_t head[4]; float maxw = 0.f, factor = 1.f, pull[12];
  bool ok = std::fread(head, 4, 4, f) == 4 && std::fread(&maxw, 4, 1, f) == 1 && std::fread(&factor, 4, 1, f) == 1 && std::fread(pull, 4, 12, f) == 12;
  se::Octree<T> dst, src;
  ok = ok && read_tree(f, dst, head[0], 0.0375f * (float)head[0]) && read_tree(f, src, head[1], 0.0375f * (float)head[1] * factor);
  std::fclose(f);
  if (!ok) return 2;
  se::merge_rule rule; rule.mode = head[2]; rule.max_weight = maxw;
  int64_t counts[10];
  se::merge_map_rigid(dst, head[3] ? dst : src, pull, rule, counts);
  /* (the trees were built from octants in any order, which merge_map_rigid must not mind; the dump is in key order: merge_map_rigid sorts
   * the destination it changed, a refused call and the source are sorted here) */
  auto by_key = [](const auto& p, const auto& q) { return p->code_ < q->code_; };
  for (se::Octree<T>* m : {&dst, &src}) {
    std::sort(m->getNodesBuffer().begin(), m->getNodesBuffer().end(), by_key);
    std::sort(m->getBlockBuffer().begin(), m->getBlockBuffer().end(), by_key);
  }
  const int64_t bad = check_tree(dst) + check_tree(src);
  FILE* o = std::fopen(out, "wb");
  if (!o) return 2;
  std::fwrite(counts, 8, 10, o);
  std::fwrite(&bad, 8, 1, o);
  write_tree(o, dst);
  write_tree(o, src);
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
