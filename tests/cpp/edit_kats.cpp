/*
 * Known-answer and randomised tests of the host restatement of se::functor::axis_aligned_map and of the edit-list function that defines
 * the device's se_hip_edit_boxes (include/se/axis_aligned.hpp).
 *
 *   edit_kats kats                 the reference's two gtest cases (se_core/test/functor/axisaligned_unittest.cpp) restated on a 256^3 map
 *                                  over 5 m with the 51^3-voxel band around the centre allocated; prints "blocks <n>", "Init <bad>",
 *                                  "BBoxTest <inside> <bad>" (bad = voxels with the wrong value)
 *   edit_kats save <file>          writes the BBoxTest map BEFORE the edit with Octree::save (the GPU test loads it and edits it there)
 *   edit_kats positions            the eight REFERENCE node positions against c0 + the closed-form offsets on nodes of every level of a
 *                                  256^3 map; prints "positions <nodes> levels <k> mismatches <m>"
 *   edit_kats random <n> <seed>    n random maps x random overlapping edit lists, SDF and OFusion, both modes, predicates on: se::apply_edits
 *                                  against a literal one-edit-at-a-time loop over axis_aligned_map(map, f, min, max), bit for bit, counts
 *                                  included; prints "checked <lists> mismatches <m>"
 */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "se/axis_aligned.hpp"

static uint64_t spread(uint64_t v) {
  uint64_t r = 0;
  for (int i = 0; i < 21; ++i) r |= ((v >> i) & 1ull) << (3 * i);
  return r;
}
static uint64_t morton(int x, int y, int z) { return spread(x) | (spread(y) << 1) | (spread(z) << 2); }
static int log2i(int s) { int l = 0; while ((1 << l) < s) ++l; return l; }

/* A map under construction: the octants that allocating blocks creates (every ancestor), appended in key order, then linked. */
template <typename T> struct Builder {
  int size;
  std::map<uint64_t, int> nodes;                 // key -> side
  std::map<uint64_t, std::vector<int>> blocks;   // key -> corner
  std::map<uint64_t, std::vector<int>> corners;  // node key -> corner
  explicit Builder(int s) : size(s) { nodes[0] = s; corners[0] = {0, 0, 0}; }
  void allocate(int x, int y, int z) {
    const int max_level = log2i(size), leaf = max_level - 3;
    for (int l = 1; l <= leaf; ++l) {
      const int side = size >> l;
      const int cx = x & ~(side - 1), cy = y & ~(side - 1), cz = z & ~(side - 1);
      const uint64_t key = morton(cx, cy, cz) | (uint64_t)l;
      if (l < leaf) { nodes[key] = side; corners[key] = {cx, cy, cz}; }
      else blocks[key] = {cx, cy, cz};
    }
  }
  std::unique_ptr<se::Octree<T>> build(float dim) const {
    std::unique_ptr<se::Octree<T>> m(new se::Octree<T>());
    m->init(size, dim);
    for (auto& n : nodes) m->add_node(n.first, (unsigned)n.second);
    for (auto& b : blocks) m->add_block(b.first, b.second.data(), false);
    m->finalize();
    return m;
  }
};

/* AxisAlignedTest::SetUp: every voxel of the band [size/2 - band/2, + band)^3, band = (int)(1 / voxelsize) */
static Builder<SDF> kat_builder() {
  const int size = 256;
  const float voxelsize = 5.f / size, inverse_voxelsize = 1.f / voxelsize;
  const int band = (int)(1 * inverse_voxelsize), offset = size / 2 - band / 2;
  Builder<SDF> b(size);
  for (int z = 0; z < band; z += 1)
    for (int y = 0; y < band; y += 1)
      for (int x = 0; x < band; x += 1) b.allocate(x + offset, y + offset, z + offset);
  return b;
}

static int run_kats() {
  auto map = kat_builder().build(5.f);
  std::printf("blocks %zu\n", map->getBlockBuffer().size());
  /* Init: assign, then read back through the same algorithm */
  const SDF seven = {7.f, 3.f};
  se::functor::axis_aligned_map(*map, [&](auto& handler, const Eigen::Vector3i&) { handler.set(seven); });
  long bad = 0, seen = 0;
  se::functor::axis_aligned_map(*map, [&](auto& handler, const Eigen::Vector3i&) { auto d = handler.get(); ++seen; if (d.x != seven.x || d.y != seven.y) ++bad; });
  for (auto& b : map->getBlockBuffer()) for (int v = 0; v < 512; ++v) if (b->voxel_block_[v].x != 7.f) ++bad;
  if (seen < (long)map->getBlockBuffer().size() * 512) ++bad;
  std::printf("Init %ld\n", bad);
  /* BBoxTest on a fresh map */
  map = kat_builder().build(5.f);
  const SDF ten = {10.f, 0.f};
  se::functor::axis_aligned_map(*map, [&](auto& handler, const Eigen::Vector3i&) { handler.set(ten); }, Eigen::Vector3i(100, 100, 100), Eigen::Vector3i(151, 151, 151));
  long inside = 0;
  bad = 0;
  for (int z = 50; z < 200; ++z)
    for (int y = 50; y < 200; ++y)
      for (int x = 50; x < 200; ++x) {
        se::VoxelBlock<SDF>* block = map->fetch(x, y, z);
        if (!block) continue;
        const bool in = x >= 100 && x <= 150 && y >= 100 && y <= 150 && z >= 100 && z <= 150;
        const float want = in ? 10.f : voxel_traits<SDF>::initValue().x;
        if (in) ++inside;
        if (block->data(x, y, z).x != want) ++bad;
      }
  std::printf("BBoxTest %ld %ld\n", inside, bad);
  return 0;
}

static int run_positions() {
  Builder<SDF> b(256);
  b.allocate(56, 12, 254); b.allocate(200, 100, 8); b.allocate(0, 0, 0); b.allocate(128, 128, 128);
  auto map = b.build(5.f);
  static const int off[8][3] = {{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {2, 2, 0}, {2, 2, 1}, {3, 2, 2}, {3, 3, 3}, {4, 4, 4}};
  long bad = 0;
  std::set<int> levels;
  for (auto& n : map->getNodesBuffer()) {
    const int level = (int)(n->code_ & 0xF);
    levels.insert(level);
    const std::vector<int>& c = b.corners.at(n->code_);
    /* the level's bits 0 and 3 are bits 0 and 1 of x, bits 1 and 4 those of y, bit 2 is bit 0 of z */
    const int c0[3] = {c[0] + ((level & 1) | (((level >> 3) & 1) << 1)), c[1] + (((level >> 1) & 1) | (((level >> 4) & 1) << 1)), c[2] + ((level >> 2) & 1)};
    const int h = (int)n->side_ / 2;
    int pos[8][3];
    se::functor::node_positions(*n, pos);
    for (int i = 0; i < 8; ++i)
      for (int k = 0; k < 3; ++k) if (pos[i][k] != c0[k] + off[i][k] * h) ++bad;
  }
  std::printf("positions %zu levels %zu mismatches %ld\n", map->getNodesBuffer().size(), levels.size(), bad);
  return bad ? 1 : 0;
}

/* ---- the literal definition: one edit after another */
template <typename T> struct Literal {
  typedef typename voxel_traits<T>::value_type value_type;
  const se_hip_edit& e;
  const se_hip_collide_test* test;
  bool reference;
  int64_t vox = 0, nod = 0;
  std::set<const void*> touched;
  bool pass(const value_type& v) const {
    if (e.only == 7u) return true;
    const value_type init = voxel_traits<T>::initValue();
    int cls;
    if (v.x == init.x && v.y == init.y) cls = 1;
    else cls = (test->occupied_above ? v.x > test->threshold : v.x < test->threshold) ? 0 : 2;
    return ((e.only >> cls) & 1u) != 0u;
  }
  value_type assign(value_type v) const {
    if (e.flags & SE_HIP_EDIT_SET_X) v.x = e.x;
    if (e.flags & SE_HIP_EDIT_SET_Y) v.y = e.y;
    return v;
  }
};

template <typename T>
static void literal_apply(se::Octree<T>& map, const se_hip_edit* edits, size_t n, const se_hip_collide_test* test, int mode, int64_t counts[4]) {
  for (int k = 0; k < 4; ++k) counts[k] = 0;
  std::set<const void*> touched;
  for (size_t i = 0; i < n; ++i) {
    const se_hip_edit& e = edits[i];
    if (!se::edit_valid<T>(e, test)) { ++counts[3]; continue; }
    Literal<T> L{e, test, mode == SE_HIP_EDIT_REFERENCE};
    /* the box as the reference takes it; blocks and (REFERENCE) nodes through axis_aligned_map, told apart by the handler's type */
    struct Op {
      Literal<T>& L;
      se::Octree<T>& map;
      void operator()(se::VoxelBlockHandler<T>& h, const Eigen::Vector3i& v) {
        if (!(L.e.flags & SE_HIP_EDIT_BLOCKS)) return;
        if (!L.pass(h.get())) return;
        h.set(L.assign(h.get()));
        ++L.vox;
        L.touched.insert(map.fetch(v(0), v(1), v(2)));
      }
      void operator()(se::NodeHandler<T>& h, const Eigen::Vector3i&) {
        if (!L.reference || !(L.e.flags & SE_HIP_EDIT_NODES)) return;
        if (!L.pass(h.get())) return;
        h.set(L.assign(h.get()));
        ++L.nod;
      }
    } op{L, map};
    se::functor::axis_aligned_map(map, op, Eigen::Vector3i(e.lo[0], e.lo[1], e.lo[2]), Eigen::Vector3i(e.hi[0], e.hi[1], e.hi[2]));
    if (!L.reference && (e.flags & SE_HIP_EDIT_NODES)) {
      /* STRICT: the child octant wholly inside [lo, hi) */
      for (auto& nd : map.getNodesBuffer()) {
        const uint64_t code = nd->code_ & ~0xFFFull;
        int c[3] = {0, 0, 0};
        for (int b = 0; b < 21; ++b) for (int k = 0; k < 3; ++k) c[k] |= (int)((code >> (3 * b + k)) & 1ull) << b;
        const int h = (int)nd->side_ / 2;
        for (int j = 0; j < 8; ++j) {
          bool in = true;
          for (int k = 0; k < 3; ++k) { const int q = c[k] + ((j >> k) & 1) * h; in = in && q >= e.lo[k] && q + h <= e.hi[k]; }
          if (!in || !L.pass(nd->value_[j])) continue;
          nd->value_[j] = L.assign(nd->value_[j]);
          ++L.nod;
        }
      }
    }
    counts[0] += L.vox; counts[1] += L.nod;
    touched.insert(L.touched.begin(), L.touched.end());
  }
  counts[2] = (int64_t)touched.size();
}

template <typename T> static bool same_maps(se::Octree<T>& a, se::Octree<T>& b) {
  if (a.getBlockBuffer().size() != b.getBlockBuffer().size() || a.getNodesBuffer().size() != b.getNodesBuffer().size()) return false;
  for (size_t i = 0; i < a.getBlockBuffer().size(); ++i)
    for (int v = 0; v < 512; ++v) {
      const auto p = a.getBlockBuffer()[i]->voxel_block_[v], q = b.getBlockBuffer()[i]->voxel_block_[v];
      if (std::memcmp(&p.x, &q.x, sizeof p.x) || std::memcmp(&p.y, &q.y, sizeof p.y)) return false;
    }
  for (size_t i = 0; i < a.getNodesBuffer().size(); ++i)
    for (int v = 0; v < 8; ++v) {
      const auto p = a.getNodesBuffer()[i]->value_[v], q = b.getNodesBuffer()[i]->value_[v];
      if (std::memcmp(&p.x, &q.x, sizeof p.x) || std::memcmp(&p.y, &q.y, sizeof p.y)) return false;
    }
  return true;
}

template <typename T> static void fill_random(se::Octree<T>& m, std::mt19937& rng, bool sdf) {
  const float xs[4] = {sdf ? 1.f : 0.f, sdf ? -0.25f : 2.5f, sdf ? 0.5f : -3.f, sdf ? 0.f : 0.75f};
  for (auto& bl : m.getBlockBuffer())
    for (int v = 0; v < 512; ++v) {
      const int r = (int)(rng() % 4);
      bl->voxel_block_[v].x = xs[r];
      bl->voxel_block_[v].y = r == 0 ? 0.f : (float)(rng() % 101);
    }
  for (auto& nd : m.getNodesBuffer())
    for (int v = 0; v < 8; ++v) { const int r = (int)(rng() % 4); nd->value_[v].x = xs[r]; nd->value_[v].y = r == 0 ? 0.f : (float)(rng() % 50); }
}

template <typename T> static long run_random_field(int n, unsigned seed, bool sdf, long& checked) {
  std::mt19937 rng(seed);
  long bad = 0;
  for (int t = 0; t < n; ++t) {
    const int size = (t % 2) ? 64 : 128;
    Builder<T> b(size);
    const int nb = 1 + (int)(rng() % 24);
    for (int i = 0; i < nb; ++i) b.allocate((int)(rng() % (size / 2)) + ((t & 2) ? 0 : size / 4), (int)(rng() % (size / 2)), (int)(rng() % size));
    std::vector<se_hip_edit> edits(40);
    std::vector<std::vector<int>> corners;
    for (auto& bl : b.blocks) corners.push_back(bl.second);
    for (auto& e : edits) {
      const bool first = &e == &edits[0];   // the whole volume, everything, first: no list is vacuous, and the later edits overwrite it
      const int kind = first ? 0 : (int)(rng() % 16);
      const std::vector<int>& near = corners[rng() % corners.size()];   // kinds 8 ..: around an allocated block, so that boxes overlap
      for (int a = 0; a < 3; ++a) {
        const int side = kind == 0 ? 2 * size : 1 + (int)(rng() % 40u);
        e.lo[a] = kind == 0 ? -size / 2 : (kind >= 8 ? near[a] + (int)(rng() % 24u) - 16 : (int)(rng() % (unsigned)(size + 40)) - 20);
        e.hi[a] = e.lo[a] + side;
      }
      if (kind == 1) e.hi[0] = e.lo[0];                 // empty
      if (kind == 2) std::swap(e.lo[1], e.hi[1]);       // inverted
      e.x = (float)((int)(rng() % 9) - 4) * 0.5f;
      e.y = (float)(rng() % 101);
      e.flags = (uint32_t)(rng() % 16);
      e.only = (rng() % 3) ? 7u : 1u + (uint32_t)(rng() % 7);
      if (first) { e.flags = 15u; e.only = 7u; }
      if (kind == 3) e.lo[2] = (1 << 30) + 1;           // invalid: coordinate
      if (kind == 4) e.flags |= 16u;                    // invalid: flag bits
      if (kind == 5) e.only = (rng() & 1) ? 0u : 8u;    // invalid: classes
      if (kind == 6) { e.flags |= SE_HIP_EDIT_SET_X; e.x = std::numeric_limits<float>::quiet_NaN(); }
      if (kind == 7) { e.flags |= SE_HIP_EDIT_SET_Y; e.y = 100.5f; }   // invalid for SDF only
    }
    const se_hip_collide_test test = {sdf ? 0.1f : 0.5f, sdf ? 0 : 1};
    for (int mode = 0; mode < 2; ++mode)
      for (int with_test = 0; with_test < 2; ++with_test) {
        auto m1 = b.build(1.f), m2 = b.build(1.f);
        std::mt19937 fr(seed * 977u + (unsigned)t);
        fill_random(*m1, fr, sdf);
        fr.seed(seed * 977u + (unsigned)t);
        fill_random(*m2, fr, sdf);
        int64_t c1[4], c2[4];
        const se_hip_collide_test* tp = with_test ? &test : nullptr;   // (null: every edit with a predicate is invalid)
        se::apply_edits(*m1, edits.data(), edits.size(), tp, mode, c1);
        literal_apply(*m2, edits.data(), edits.size(), tp, mode, c2);
        ++checked;
        if (!same_maps(*m1, *m2) || std::memcmp(c1, c2, sizeof c1)) {
          if (bad < 5) std::fprintf(stderr, "map %d mode %d test %d: counts %lld %lld %lld %lld vs %lld %lld %lld %lld\n", t, mode, with_test, (long long)c1[0], (long long)c1[1],
                                    (long long)c1[2], (long long)c1[3], (long long)c2[0], (long long)c2[1], (long long)c2[2], (long long)c2[3]);
          ++bad;
        }
        if (with_test && (c1[0] == 0 || c1[1] == 0)) { std::fprintf(stderr, "map %d mode %d: a vacuous list (%lld voxel, %lld node applications)\n", t, mode, (long long)c1[0], (long long)c1[1]); ++bad; }
      }
  }
  return bad;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "kats";
  if (mode == "kats") return run_kats();
  if (mode == "save") {
    if (argc < 3) return 2;
    kat_builder().build(5.f)->save(argv[2]);
    return 0;
  }
  if (mode == "positions") return run_positions();
  if (mode == "random") {
    const int n = argc > 2 ? std::atoi(argv[2]) : 10;
    const unsigned seed = argc > 3 ? (unsigned)std::atoi(argv[3]) : 1u;
    long checked = 0;
    const long bad = run_random_field<SDF>(n, seed, true, checked) + run_random_field<OFusion>(n, seed + 1, false, checked);
    std::printf("checked %ld mismatches %ld\n", checked, bad);
    return bad ? 1 : 0;
  }
  return 2;
}
