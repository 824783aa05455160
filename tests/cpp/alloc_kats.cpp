/*
 * Tests of se::allocate_boxes (include/se/allocate_region.hpp), the host restatement that defines the device's se_hip_allocate_boxes.
 *
 *   alloc_kats random <n> <seed>         n random start maps (some blocks inactive, some values changed) x random box lists, SDF and OFusion:
 *                                        leaf and coarse levels, overlapping and repeated boxes, boxes clipped by the volume or wholly
 *                                        outside, empty and inverted boxes, every invalid rule.  allocate_boxes against a literal truth --
 *                                        every octant of the level is tested against the clipped box, its key and the keys of its ancestors
 *                                        go into a set --: octant sets, counts, what new_keys guarantees, initValue() and active_ of what is new,
 *                                        every bit of what existed, the links of the tree.  Prints "checked <lists> mismatches <m>".
 *   alloc_kats dump <size> <in> <out>    in: se_hip_alloc_box records; allocate_boxes on the empty map of that size; out: int64 counts[4],
 *                                        uint64 nb, block keys, uint64 nn, node keys (root included), uint64 nk, new_keys -- each list sorted
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <random>
#include <set>
#include <vector>

#include "se/allocate_region.hpp"

static uint64_t spread(uint64_t v) {
  uint64_t r = 0;
  for (int i = 0; i < 21; ++i) r |= ((v >> i) & 1ull) << (3 * i);
  return r;
}
static uint64_t morton(int x, int y, int z) { return spread(x) | (spread(y) << 1) | (spread(z) << 2); }
static int log2i(int s) { int l = 0; while ((1 << l) < s) ++l; return l; }

/* the literal definition: the keys a list requests, and their ancestor closure */
struct Truth { std::set<uint64_t> requested, closure; long pairs = 0, invalid = 0; };
static Truth literal(int size, const std::vector<se_hip_alloc_box>& boxes) {
  Truth t;
  const int leaf = log2i(size) - 3;
  const long limit = 1l << 30;
  for (const se_hip_alloc_box& b : boxes) {
    bool ok = b.reserved == 0 && b.level >= 0 && b.level <= leaf;
    for (int k = 0; k < 3; ++k) ok = ok && b.lo[k] >= -limit && b.lo[k] <= limit && b.hi[k] >= -limit && b.hi[k] <= limit;
    if (!ok) { ++t.invalid; continue; }
    const int level = b.level == 0 ? leaf : b.level, side = size >> level, cells = 1 << level;
    for (int z = 0; z < cells; ++z)
      for (int y = 0; y < cells; ++y)
        for (int x = 0; x < cells; ++x) {
          const int c[3] = {x * side, y * side, z * side};
          bool hit = true;   /* the cube [c, c + side) meets [lo, hi) n [0, size): some voxel lies in both */
          for (int k = 0; k < 3; ++k) {
            const long lo = std::max<long>(std::max<long>(b.lo[k], 0), c[k]), hi = std::min<long>(std::min<long>(b.hi[k], size), c[k] + side);
            hit = hit && lo < hi;
          }
          if (!hit) continue;
          ++t.pairs;
          t.requested.insert(morton(c[0], c[1], c[2]) | (uint64_t)level);
          for (int l = level; l >= 1; --l) {
            const int s = size >> l;
            t.closure.insert(morton(c[0] / s * s, c[1] / s * s, c[2] / s * s) | (uint64_t)l);
          }
        }
  }
  return t;
}

template <typename T> static void set_value(typename voxel_traits<T>::value_type& v, float x, float y) { v.x = x; v.y = y; }

template <typename T> static long run_one(std::mt19937& rng, int size) {
  typedef typename voxel_traits<T>::value_type V;
  const int leaf = log2i(size) - 3;
  /* the start map: the ancestor closure of some random blocks, values and flags changed */
  std::map<uint64_t, std::vector<int>> octants;   /* key -> corner */
  octants[0] = {0, 0, 0};
  const int nstart = (int)(rng() % 40);
  for (int i = 0; i < nstart; ++i) {
    const int p[3] = {(int)(rng() % size), (int)(rng() % size), (int)(rng() % size)};
    for (int l = 1; l <= leaf; ++l) {
      const int s = size >> l;
      octants[morton(p[0] / s * s, p[1] / s * s, p[2] / s * s) | (uint64_t)l] = {p[0] / s * s, p[1] / s * s, p[2] / s * s};
    }
  }
  se::Octree<T> map;
  map.init(size, 5.f);
  std::map<uint64_t, std::vector<float>> before;   /* key -> values (x, y interleaved), then the active flag for blocks */
  for (auto& o : octants) {
    const int level = (int)(o.first & 0x1FF);
    if (level == leaf) {
      auto* b = map.add_block(o.first, o.second.data(), rng() % 2 == 0);
      for (int v = 0; v < 512; ++v) if (rng() % 4 == 0) set_value<T>(b->voxel_block_[v], (float)(rng() % 7) - 3.f, (float)(rng() % 50));
    } else {
      auto* nd = map.add_node(o.first, (unsigned)(size >> level));
      for (int v = 0; v < 8; ++v) if (rng() % 2 == 0) set_value<T>(nd->value_[v], (float)(rng() % 7) - 3.f, (float)(rng() % 50));
    }
  }
  map.finalize();
  for (auto& b : map.getBlockBuffer()) { auto& r = before[b->code_]; for (auto& v : b->voxel_block_) { r.push_back(v.x); r.push_back((float)v.y); } r.push_back(b->active_ ? 1.f : 0.f); }
  for (auto& nd : map.getNodesBuffer()) { auto& r = before[nd->code_]; for (auto& v : nd->value_) { r.push_back(v.x); r.push_back((float)v.y); } }
  /* the list */
  std::vector<se_hip_alloc_box> boxes;
  auto add = [&](int x, int y, int z, int a, int b, int c, int level) {
    se_hip_alloc_box r;
    r.lo[0] = x; r.lo[1] = y; r.lo[2] = z; r.hi[0] = x + a; r.hi[1] = y + b; r.hi[2] = z + c; r.level = level; r.reserved = 0;
    boxes.push_back(r);
  };
  auto any = [&](int m) { return (int)(rng() % (unsigned)(size + 2 * m)) - m; };
  const int nb = 1 + (int)(rng() % 12);
  for (int i = 0; i < nb; ++i) {
    const int level = rng() % 2 ? 0 : (int)(rng() % (unsigned)(leaf + 1));
    add(any(24), any(24), any(24), 1 + (int)(rng() % 40), 1 + (int)(rng() % 40), 1 + (int)(rng() % 40), level);
    if (rng() % 3 == 0) boxes.push_back(boxes.back());                                             /* a repeated box */
    if (rng() % 3 == 0) { se_hip_alloc_box o = boxes.back(); o.lo[0] += 5; o.hi[1] += 9; o.level = (int)(rng() % (unsigned)(leaf + 1)); boxes.push_back(o); }   /* an overlapping one, any level */
  }
  add(size - 3, size - 3, size - 3, 40, 40, 40, 0);          /* clipped by the upper faces */
  add(-30, -30, 4, 33, 33, 3, (int)(rng() % (unsigned)(leaf + 1)));   /* clipped by the lower faces */
  add(size, 0, 0, 16, 16, 16, 0); add(-16, 0, 0, 16, 16, 16, 1);   /* wholly outside */
  add(10, 10, 10, 0, 9, 9, 0); add(40, 40, 40, -9, 9, 9, 2);   /* empty, inverted */
  if (rng() % 4 == 0) add(-size, -size, -size, 3 * size, 3 * size, 3 * size, 1 + (int)(rng() % (unsigned)leaf));   /* the whole volume, coarse or leaf */
  /* every invalid rule */
  add(0, 0, 0, 8, 8, 8, 0); boxes.back().lo[1] = -(1 << 30) - 1;
  add(0, 0, 0, 8, 8, 8, 0); boxes.back().hi[2] = (1 << 30) + 1;
  add(0, 0, 0, 8, 8, 8, -1);
  add(0, 0, 0, 8, 8, 8, leaf + 1);
  add(0, 0, 0, 8, 8, 8, 0); boxes.back().reserved = 1u;
  std::shuffle(boxes.begin(), boxes.end(), rng);

  const Truth t = literal(size, boxes);
  int64_t counts[4] = {-1, -1, -1, -1};
  std::vector<se::key_t> keys;
  se::allocate_boxes(map, boxes.data(), boxes.size(), counts, &keys);

  long bad = 0;
  std::set<uint64_t> want;
  for (auto& o : octants) want.insert(o.first);
  long new_blocks = 0, new_nodes = 0;
  for (uint64_t k : t.closure) if (want.insert(k).second) { if ((int)(k & 0x1FF) == leaf) ++new_blocks; else ++new_nodes; }
  std::set<uint64_t> got;
  uint64_t prev = 0;
  bool first = true;
  auto ordered = [&](uint64_t k) { if (!first && k <= prev) ++bad; prev = k; first = false; };
  for (auto& nd : map.getNodesBuffer()) { got.insert(nd->code_); ordered(nd->code_); }
  first = true;
  for (auto& b : map.getBlockBuffer()) { got.insert(b->code_); ordered(b->code_); }
  if (got != want) ++bad;
  if (counts[0] != new_blocks || counts[1] != new_nodes || counts[2] != t.pairs || counts[3] != t.invalid || t.invalid != 5) ++bad;
  /* new_keys: requested octants that did not exist, none twice, and together with the map before they imply the map after (a requested
   * octant that came into being as the ancestor of a finer request need not be listed: which of the two came first is unspecified) */
  std::set<uint64_t> kset(keys.begin(), keys.end()), implied;
  for (auto& o : octants) implied.insert(o.first);
  for (uint64_t k : keys) {
    if (!t.requested.count(k) || octants.count(k)) ++bad;
    const int level = (int)(k & 0x1FF);
    for (int l = level; l >= 1; --l) implied.insert(((k & ~0x1FFull) & ~((1ull << (3 * (log2i(size) - l))) - 1ull)) | (uint64_t)l);
  }
  if (kset.size() != keys.size() || implied != got) ++bad;
  /* values, flags, links */
  const V init = voxel_traits<T>::initValue();
  for (auto& b : map.getBlockBuffer()) {
    auto it = before.find(b->code_);
    const int* c = b->coordinates();
    if (map.fetch(c[0], c[1], c[2]) != b.get() || b->code_ != (morton(c[0], c[1], c[2]) | (uint64_t)leaf)) ++bad;
    for (int v = 0; v < 512; ++v) {
      const float wx = it == before.end() ? init.x : it->second[2 * v], wy = it == before.end() ? (float)init.y : it->second[2 * v + 1];
      const float gy = (float)b->voxel_block_[v].y;
      if (std::memcmp(&b->voxel_block_[v].x, &wx, 4) || std::memcmp(&gy, &wy, 4)) ++bad;
    }
    if (b->active_ != (it == before.end() ? true : it->second[1024] != 0.f)) ++bad;
  }
  for (auto& nd : map.getNodesBuffer()) {
    auto it = before.find(nd->code_);
    const int level = (int)(nd->code_ & 0x1FF);
    if ((int)nd->side_ != size >> level) ++bad;
    for (int v = 0; v < 8; ++v) {
      const float wx = it == before.end() ? init.x : it->second[2 * v], wy = it == before.end() ? (float)init.y : it->second[2 * v + 1];
      const float gy = (float)nd->value_[v].y;
      if (std::memcmp(&nd->value_[v].x, &wx, 4) || std::memcmp(&gy, &wy, 4)) ++bad;
    }
  }
  /* a second identical call creates nothing */
  int64_t again[4];
  se::allocate_boxes(map, boxes.data(), boxes.size(), again, &keys);
  if (again[0] != 0 || again[1] != 0 || again[2] != counts[2] || again[3] != counts[3] || !keys.empty()) ++bad;
  return bad;
}

static int run_dump(int size, const char* in, const char* out) {
  FILE* f = std::fopen(in, "rb");
  if (!f) return 2;
  std::vector<se_hip_alloc_box> boxes;
  se_hip_alloc_box b;
  while (std::fread(&b, sizeof b, 1, f) == 1) boxes.push_back(b);
  std::fclose(f);
  se::Octree<SDF> map;
  map.init(size, 5.f);
  int64_t counts[4];
  std::vector<se::key_t> keys;
  se::allocate_boxes(map, boxes.data(), boxes.size(), counts, &keys);
  std::sort(keys.begin(), keys.end());
  std::vector<uint64_t> bk, nk;
  for (auto& p : map.getBlockBuffer()) bk.push_back(p->code_);
  for (auto& p : map.getNodesBuffer()) nk.push_back(p->code_);
  FILE* o = std::fopen(out, "wb");
  if (!o) return 2;
  std::fwrite(counts, 8, 4, o);
  const std::vector<uint64_t> ks(keys.begin(), keys.end());
  const std::vector<uint64_t>* lists[3] = {&bk, &nk, &ks};
  for (const std::vector<uint64_t>* v : lists) {
    const uint64_t n = v->size();
    std::fwrite(&n, 8, 1, o);
    if (n) std::fwrite(v->data(), 8, n, o);
  }
  std::fclose(o);
  return 0;
}

int main(int argc, char** argv) {
  static_assert(sizeof(se_hip_alloc_box) == 32, "se_hip_alloc_box is 32 bytes");
  if (argc >= 4 && !std::strcmp(argv[1], "random")) {
    std::mt19937 rng((unsigned)std::atoi(argv[3]));
    const int n = std::atoi(argv[2]);
    long bad = 0, lists = 0;
    for (int i = 0; i < n; ++i) {
      const int size = i % 3 == 0 ? 128 : 64;
      bad += run_one<SDF>(rng, size); ++lists;
      bad += run_one<OFusion>(rng, size); ++lists;
    }
    std::printf("checked %ld mismatches %ld\n", lists, bad);
    return 0;
  }
  if (argc >= 5 && !std::strcmp(argv[1], "dump")) return run_dump(std::atoi(argv[2]), argv[3], argv[4]);
  std::fprintf(stderr, "usage: %s random <n> <seed> | dump <size> <boxes.bin> <out.bin>\n", argv[0]);
  return 2;
}
