/*
 * Known-answer tests of se::geometry::collides_with on the host mirror (include/se/octree_collision.hpp), and a randomised check of the
 * closed form that the device's SE_HIP_COLLIDE_REFERENCE mode evaluates against the literal traversal.
 *
 *   collision_kats kats               the reference's five gtest cases (se_core/test/geometry/octree_collision_unittest.cpp) restated,
 *                                     plus three quirk cases that separate the reference's answer from the strict one; one line per case:
 *                                     "<name> <reference status> <strict status>" (0 occupied, 1 unseen, 2 empty)
 *   collision_kats save <dir>         writes the maps of those cases with Octree::save (<dir>/<map>.bin) and prints their names
 *   collision_kats random <n> <seed>  n random maps x boxes: literal traversal vs closed form; prints "checked <k> mismatches <m>"
 *
 * The maps are 256^3 SDF octrees over 5 m.  The reference's test field is a float with initValue 1 and a test functor that calls 1 unseen,
 * 10 empty and anything else occupied; here the value is SDF's {x, y} with y = 0 and the classification is voxel_test<SDF>{5, below}:
 * {1, 0} unseen, x = 10 empty, x = 2 occupied -- the same answers.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "se/octree.hpp"
#include "se/octree_collision.hpp"

using se::geometry::collision_status;
using se::geometry::int3;
typedef se::Octree<SDF> Map;

static uint64_t spread(uint64_t v) {
  uint64_t r = 0;
  for (int i = 0; i < 21; ++i) r |= ((v >> i) & 1ull) << (3 * i);
  return r;
}
static uint64_t morton(int x, int y, int z) { return spread(x) | (spread(y) << 1) | (spread(z) << 2); }
static int compact(uint64_t code, int axis) {
  int v = 0;
  for (int i = 0; i < 21; ++i) v |= (int)((code >> (3 * i + axis)) & 1ull) << i;
  return v;
}
static int log2i(int s) { int l = 0; while ((1 << l) < s) ++l; return l; }

/* A map under construction: the octants that allocating `blocks` creates (every ancestor), appended in key order, then linked. */
struct Builder {
  int size;
  std::map<uint64_t, int> nodes;                 // key -> side
  std::map<uint64_t, std::vector<int>> blocks;   // key -> corner
  explicit Builder(int s) : size(s) { nodes[0] = s; }
  void allocate(int x, int y, int z) {
    const int max_level = log2i(size), leaf = max_level - 3;
    for (int l = 1; l <= leaf; ++l) {
      const int side = size >> l;
      const int cx = x & ~(side - 1), cy = y & ~(side - 1), cz = z & ~(side - 1);
      const uint64_t key = morton(cx, cy, cz) | (uint64_t)l;
      if (l < leaf) nodes[key] = side;
      else blocks[key] = {cx, cy, cz};
    }
  }
  std::unique_ptr<Map> build(float dim) const {
    std::unique_ptr<Map> m(new Map());
    m->init(size, dim);
    for (auto& n : nodes) m->add_node(n.first, (unsigned)n.second);
    for (auto& b : blocks) m->add_block(b.first, b.second.data(), false);
    m->finalize();
    return m;
  }
};

/* se::functor::axis_aligned_map over [0, size]: every voxel of every block, then every node's eight values -- each at the corner the
 * reference computes: unpack_morton(code_) (the level bits included) plus the running sum of dir(i) * side / 2 over i (cumulative). */
template <typename F>
static void axis_aligned_map(Map& m, F f) {
  const int size = m.size();
  for (auto& b : m.getBlockBuffer()) {
    const int* c = b->coordinates();
    for (int z = c[2]; z < c[2] + 8; ++z)
      for (int y = c[1]; y < c[1] + 8; ++y)
        for (int x = c[0]; x < c[0] + 8; ++x) {
          if (!(x < size && y < size && z < size)) continue;
          f(b->voxel_block_[(x - c[0]) + 8 * (y - c[1]) + 64 * (z - c[2])], x, y, z);
        }
  }
  for (auto& n : m.getNodesBuffer()) {
    int v[3] = {compact(n->code_, 0), compact(n->code_, 1), compact(n->code_, 2)};
    for (int i = 0; i < 8; ++i) {
      const int h = (int)n->side_ / 2;
      v[0] += ((i & 1) ? 1 : 0) * h; v[1] += ((i & 2) ? 1 : 0) * h; v[2] += ((i & 4) ? 1 : 0) * h;
      bool in = true;
      for (int k = 0; k < 3; ++k) in = in && v[k] >= 0 && v[k] <= size;
      if (!in) continue;
      f(n->value_[i], v[0], v[1], v[2]);
    }
  }
}

static const se::geometry::voxel_test<SDF> kTest = {5.f, false};

/* strict mode by brute force over Octree::get: min over [lo, lo + side) of the class, outside the volume unseen */
static int strict_brute(const Map& m, const int lo[3], const int side[3]) {
  int st = 2;
  for (int z = lo[2]; z < lo[2] + side[2]; ++z)
    for (int y = lo[1]; y < lo[1] + side[1]; ++y)
      for (int x = lo[0]; x < lo[0] + side[0]; ++x) {
        const bool in = x >= 0 && y >= 0 && z >= 0 && x < m.size() && y < m.size() && z < m.size();
        const int c = in ? (int)kTest(m.get(x, y, z)) : 1;
        if (c < st) st = c;
      }
  return st;
}

struct Case { std::string name, map; int lo[3], side[3]; };

/* the maps of the cases */
static std::map<std::string, std::unique_ptr<Map>> kat_maps() {
  std::map<std::string, std::unique_ptr<Map>> maps;
  auto set_to_ten = [](SDF& v, int x, int y, int z) { if (x >= 48 && y >= 0 && z >= 240) v.x = 10.f; };
  Builder kb(256);
  kb.allocate(56, 12, 254);
  maps["kat"] = kb.build(5.f);
  axis_aligned_map(*maps["kat"], set_to_ten);
  /* Collision: then every voxel and node value set to 2 */
  maps["kat_collision"] = kb.build(5.f);
  axis_aligned_map(*maps["kat_collision"], set_to_ten);
  axis_aligned_map(*maps["kat_collision"], [](SDF& v, int, int, int) { v.x = 2.f; });
  /* CollisionFreeLeaf: the block's voxels rewritten (x < xlast / 2 etc. never holds there: all 10) */
  maps["kat_freeleaf"] = kb.build(5.f);
  axis_aligned_map(*maps["kat_freeleaf"], set_to_ten);
  {
    se::VoxelBlock<SDF>* b = maps["kat_freeleaf"]->fetch(56, 12, 254);
    const int* c = b->coordinates();
    const int xl = c[0] + 8, yl = c[1] + 8, zl = c[2] + 8;
    for (int z = c[2]; z < zl; ++z)
      for (int y = c[1]; y < yl; ++y)
        for (int x = c[0]; x < xl; ++x)
          b->voxel_block_[(x - c[0]) + 8 * (y - c[1]) + 64 * (z - c[2])].x = (x < xl / 2 && y < yl / 2 && z < zl / 2) ? 2.f : 10.f;
  }
  /* quirk 1: blocks (0,0,0) all empty and (8,0,0) empty but for one occupied voxel (9,1,1) */
  Builder q1(256);
  q1.allocate(0, 0, 0); q1.allocate(8, 0, 0);
  maps["q_order"] = q1.build(5.f);
  for (auto& b : maps["q_order"]->getBlockBuffer())
    for (int v = 0; v < 512; ++v) b->voxel_block_[v].x = 10.f;
  maps["q_order"]->fetch(8, 0, 0)->voxel_block_[1 + 8 * 1 + 64 * 1].x = 2.f;
  /* quirk 2: block (0,0,0) only; its parent (side 16) has value_[0] empty and value_[1] occupied */
  Builder q2(256);
  q2.allocate(0, 0, 0);
  maps["q_slot0"] = q2.build(5.f);
  for (auto& b : maps["q_slot0"]->getBlockBuffer())
    for (int v = 0; v < 512; ++v) b->voxel_block_[v].x = 10.f;
  {
    se::Node<SDF>* n = maps["q_slot0"]->fetch_octant(0, 0, 0, 4);
    n->value_[0].x = 10.f;
    n->value_[1].x = 2.f;
  }
  /* quirk 3: block (0,0,0) all empty but for one occupied voxel (4,4,4) */
  maps["q_inclusive"] = q2.build(5.f);
  for (auto& b : maps["q_inclusive"]->getBlockBuffer())
    for (int v = 0; v < 512; ++v) b->voxel_block_[v].x = 10.f;
  maps["q_inclusive"]->fetch(0, 0, 0)->voxel_block_[4 + 8 * 4 + 64 * 4].x = 2.f;
  return maps;
}

static const Case kCases[] = {
    {"TotallyUnseen", "kat", {23, 0, 100}, {2, 2, 2}},
    {"PartiallyUnseen", "kat", {47, 0, 239}, {6, 6, 6}},
    {"Empty", "kat", {49, 1, 242}, {1, 1, 1}},
    {"Collision", "kat_collision", {54, 10, 249}, {5, 5, 3}},
    {"CollisionFreeLeaf", "kat_freeleaf", {61, 13, 253}, {2, 2, 2}},
    {"QuirkLeafOrder", "q_order", {4, 0, 0}, {8, 4, 4}},
    {"QuirkParentSlot0", "q_slot0", {9, 0, 0}, {2, 2, 2}},
    {"QuirkInclusive", "q_inclusive", {2, 2, 2}, {2, 2, 2}},
};

/* ---- the closed form of the reference traversal, evaluated from its definition (independent of the stack walk) */
struct Oct { se::Node<SDF>* n; int x, y, z, side; };
static bool ref_overlap(const int lo[3], const int side[3], int x, int y, int z, int s) {
  const int3 a = {{lo[0], lo[1], lo[2]}}, ae = {{side[0], side[1], side[2]}}, b = {{x, y, z}}, be = {{s, s, s}};
  return se::geometry::aabb_aabb_collision(a, ae, b, be) != 0;
}
static int closed_form(const Map& m, const int lo[3], const int side[3]) {
  // visited octants: the root, and every octant whose ancestors below the root and itself overlap (walked top-down here)
  std::vector<Oct> visited, stack = {{m.root(), 0, 0, 0, m.size()}};
  while (!stack.empty()) {
    Oct o = stack.back(); stack.pop_back();
    visited.push_back(o);
    const int h = o.side / 2;
    for (int i = 0; i < 8; ++i) {
      se::Node<SDF>* c = o.n->child(i);
      const int x = o.x + ((i & 1) ? h : 0), y = o.y + ((i & 2) ? h : 0), z = o.z + ((i & 4) ? h : 0);
      if (c && ref_overlap(lo, side, x, y, z, h)) stack.push_back({c, x, y, z, h});
    }
  }
  const Oct* best = nullptr;
  for (auto& o : visited)
    if (o.n->isLeaf() && (!best || morton(o.x, o.y, o.z) < morton(best->x, best->y, best->z))) best = &o;
  int st = 2;
  if (best) st = (int)se::geometry::collides_with(static_cast<const se::VoxelBlock<SDF>*>(best->n), int3{{lo[0], lo[1], lo[2]}},
                                                 int3{{side[0], side[1], side[2]}}, kTest);
  const uint64_t code_best = best ? morton(best->x, best->y, best->z) : 0;
  for (auto& o : visited) {
    if (o.n->isLeaf() || o.n->children_mask_ == 0) continue;
    // counts if Q is not an ancestor of L* and code(Q) < code(L*): its octant ends at or before L*'s code
    const uint64_t end = morton(o.x, o.y, o.z) + (uint64_t)o.side * o.side * o.side;
    if (best && end > code_best) continue;
    const int h = o.side / 2;
    bool ev = false;
    for (int i = 0; i < 8; ++i)
      if (!o.n->child(i) && ref_overlap(lo, side, o.x + ((i & 1) ? h : 0), o.y + ((i & 2) ? h : 0), o.z + ((i & 4) ? h : 0), h)) ev = true;
    if (ev) { const int c = (int)kTest(o.n->value_[0]); if (c < st) st = c; }
  }
  return st;
}

static int literal(const Map& m, const int lo[3], const int side[3]) {
  return (int)se::geometry::collides_with(m, int3{{lo[0], lo[1], lo[2]}}, int3{{side[0], side[1], side[2]}}, kTest);
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "kats";
  if (mode == "kats" || mode == "save") {
    auto maps = kat_maps();
    if (mode == "save") {
      if (argc < 3) return 2;
      for (auto& m : maps) { m.second->save(std::string(argv[2]) + "/" + m.first + ".bin"); std::printf("%s\n", m.first.c_str()); }
      return 0;
    }
    for (const Case& c : kCases) {
      const Map& m = *maps[c.map];
      const int r = literal(m, c.lo, c.side), cf = closed_form(m, c.lo, c.side);
      if (r != cf) { std::fprintf(stderr, "%s: literal %d closed form %d\n", c.name.c_str(), r, cf); return 1; }
      std::printf("%s %d %d\n", c.name.c_str(), r, strict_brute(m, c.lo, c.side));
    }
    return 0;
  }
  if (mode == "random") {
    const int n = argc > 2 ? std::atoi(argv[2]) : 20;
    std::mt19937 rng(argc > 3 ? (unsigned)std::atoi(argv[3]) : 1u);
    const float vals[3] = {1.f, 2.f, 10.f};   // unseen, occupied, empty
    long checked = 0, bad = 0;
    for (int t = 0; t < n; ++t) {
      const int size = (t % 2) ? 64 : 128;
      Builder b(size);
      const int nb = 1 + (int)(rng() % 24);
      // clustered blocks, so that boxes meet several of them
      for (int i = 0; i < nb; ++i) b.allocate((int)(rng() % (size / 2)) + ((t & 2) ? 0 : size / 4), (int)(rng() % (size / 2)), (int)(rng() % size));
      auto m = b.build(1.f);
      for (auto& bl : m->getBlockBuffer())
        for (int v = 0; v < 512; ++v) { const int r = (int)(rng() % 64); bl->voxel_block_[v].x = vals[r == 0 ? 1 : (r < 8 ? 0 : 2)]; }
      for (auto& nd : m->getNodesBuffer())
        for (int v = 0; v < 8; ++v) nd->value_[v].x = vals[rng() % 3];
      for (int k = 0; k < 400; ++k) {
        int lo[3], side[3];
        for (int a = 0; a < 3; ++a) {
          side[a] = 1 + (int)(rng() % ((k % 4 == 0) ? (unsigned)size : 20u));
          lo[a] = (int)(rng() % (unsigned)(size + 40)) - 20;
        }
        const int r = literal(*m, lo, side), cf = closed_form(*m, lo, side);
        ++checked;
        if (r != cf) {
          if (bad < 5) std::fprintf(stderr, "map %d box (%d %d %d | %d %d %d): literal %d closed form %d\n", t, lo[0], lo[1], lo[2], side[0], side[1], side[2], r, cf);
          ++bad;
        }
      }
    }
    std::printf("checked %ld mismatches %ld\n", checked, bad);
    return bad ? 1 : 0;
  }
  return 2;
}
