/*
 * Known-answer and randomised tests of the motion collision queries on the host mirror (include/se/motion_collision.hpp): the recursive
 * traversal against the literal definition (every voxel of the motion's bounding box), in status and in the exact rational of t_first.
 *
 *   motion_kats kats               hand-worked cases on 64^3 SDF maps; one line per case:
 *                                  "<name> <valid> <status, stop_at occupied> <num> <den> <status, stop_at unseen> <num> <den>"
 *                                  (0 occupied, 1 unseen, 2 empty; num / den in lowest terms, 2 / 1 = free, -1 / 1 = invalid).  A case whose
 *                                  traversal and brute force differ, or whose d = 0 answer differs from the strict box, ends the program with 1.
 *   motion_kats random <n> <seed>  n random 64^3 maps (both fields in turn) x 400 motions; prints "checked <k> mismatches <m>"
 *
 * Values: x = 10 empty, x = 2 occupied, initValue() unseen, judged by voxel_test{5, below} (as tests/cpp/collision_kats.cpp).
 */
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "se/motion_collision.hpp"
#include "se/octree.hpp"
#include "se/octree_collision.hpp"

using se::geometry::collision_status;
using se::geometry::int3;
using se::geometry::motion_result;

static uint64_t spread(uint64_t v) {
  uint64_t r = 0;
  for (int i = 0; i < 21; ++i) r |= ((v >> i) & 1ull) << (3 * i);
  return r;
}
static uint64_t morton(int x, int y, int z) { return spread(x) | (spread(y) << 1) | (spread(z) << 2); }
static int log2i(int s) { int l = 0; while ((1 << l) < s) ++l; return l; }

/* A map under construction: the octants that allocating `blocks` creates (every ancestor), appended in key order, then linked. */
template <typename T>
struct Builder {
  int size;
  std::map<uint64_t, int> nodes;                 // key -> side
  std::map<uint64_t, std::vector<int>> blocks;   // key -> corner
  explicit Builder(int s) : size(s) { nodes[0] = s; }
  void allocate(int x, int y, int z) {
    const int leaf = log2i(size) - 3;
    for (int l = 1; l <= leaf; ++l) {
      const int side = size >> l;
      const int cx = x & ~(side - 1), cy = y & ~(side - 1), cz = z & ~(side - 1);
      const uint64_t key = morton(cx, cy, cz) | (uint64_t)l;
      if (l < leaf) nodes[key] = side;
      else blocks[key] = {cx, cy, cz};
    }
  }
  std::unique_ptr<se::Octree<T>> build() const {
    std::unique_ptr<se::Octree<T>> m(new se::Octree<T>());
    m->init(size, 1.f);
    for (auto& n : nodes) m->add_node(n.first, (unsigned)n.second);
    for (auto& b : blocks) m->add_block(b.first, b.second.data(), false);
    m->finalize();
    return m;
  }
};

typedef se::Octree<SDF> Map;
static const se::geometry::voxel_test<SDF> kTest = {5.f, false};

/* a 64^3 map with every block allocated and every voxel empty, then the listed voxels occupied */
static std::unique_ptr<Map> free_map(const std::vector<int3>& occupied) {
  Builder<SDF> b(64);
  for (int z = 0; z < 64; z += 8)
    for (int y = 0; y < 64; y += 8)
      for (int x = 0; x < 64; x += 8) b.allocate(x, y, z);
  auto m = b.build();
  for (auto& bl : m->getBlockBuffer())
    for (int v = 0; v < 512; ++v) bl->voxel_block_[v].x = 10.f;
  for (const int3& o : occupied) {
    se::VoxelBlock<SDF>* bl = m->fetch(o(0), o(1), o(2));
    bl->voxel_block_[(o(0) & 7) + 8 * (o(1) & 7) + 64 * (o(2) & 7)].x = 2.f;
  }
  return m;
}

static int strict_brute(const Map& m, const int3& lo, const int3& side) {
  int st = 2;
  for (int z = lo(2); z < lo(2) + side(2); ++z)
    for (int y = lo(1); y < lo(1) + side(1); ++y)
      for (int x = lo(0); x < lo(0) + side(0); ++x) {
        const bool in = x >= 0 && y >= 0 && z >= 0 && x < m.size() && y < m.size() && z < m.size();
        const int c = in ? (int)kTest(m.get(x, y, z)) : 1;
        if (c < st) st = c;
      }
  return st;
}

struct Case { std::string name, map; int3 lo, side, d; };

template <typename T, typename TestF>
static bool same(const se::Octree<T>& m, const int3& lo, const int3& side, const int3& d, TestF test, collision_status stop, motion_result* out) {
  const motion_result a = se::geometry::motion_status_and_entry(m, lo, side, d, test, stop);
  const motion_result b = se::geometry::motion_status_and_entry_brute(m, lo, side, d, test, stop);
  if (out) *out = a;
  if (a.valid != b.valid) return false;
  if (!a.valid) return a.t_first.num == b.t_first.num && a.t_first.den == b.t_first.den;
  return a.status == b.status && a.t_first.num == b.t_first.num && a.t_first.den == b.t_first.den;
}

static int run_kats() {
  std::map<std::string, std::unique_ptr<Map>> maps;
  maps["a"] = free_map({{{10, 10, 10}}});
  maps["b"] = free_map({{{10, 11, 0}}});
  maps["c"] = free_map({{{10, 12, 0}}});
  maps["d"] = free_map({{{10, 5, 5}}});
  {   // a wall: every voxel of the plane x = 20
    std::vector<int3> w;
    for (int z = 0; z < 64; ++z)
      for (int y = 0; y < 64; ++y) w.push_back({{20, y, z}});
    maps["wall"] = free_map(w);
  }
  maps["free"] = free_map({});
  {   // the block at (24, 0, 0) never observed, an obstacle behind it
    maps["gap"] = free_map({{{40, 3, 3}}});
    se::VoxelBlock<SDF>* bl = maps["gap"]->fetch(24, 0, 0);
    for (int v = 0; v < 512; ++v) bl->voxel_block_[v] = voxel_traits<SDF>::initValue();
  }
  const int lim = se::geometry::motion_limit;
  const Case cases[] = {
      {"Diagonal3", "a", {{0, 0, 0}}, {{1, 1, 1}}, {{20, 20, 20}}},
      {"DiagonalTouches", "b", {{0, 0, 0}}, {{1, 1, 1}}, {{20, 20, 0}}},
      {"DiagonalOpenEnd", "c", {{0, 0, 0}}, {{1, 1, 1}}, {{20, 20, 0}}},
      {"SlideAlongWall", "wall", {{19, 5, 5}}, {{1, 2, 2}}, {{0, 30, 7}}},
      {"SlideAlongWallFar", "wall", {{21, 40, 40}}, {{3, 2, 2}}, {{0, -30, -7}}},
      {"IntoWall", "wall", {{10, 5, 5}}, {{2, 2, 2}}, {{16, 30, 0}}},
      {"ZeroMotion", "a", {{8, 9, 9}}, {{3, 3, 3}}, {{0, 0, 0}}},
      {"ZeroMotionFree", "a", {{11, 9, 9}}, {{3, 3, 3}}, {{0, 0, 0}}},
      {"LeaveXlo", "free", {{30, 30, 30}}, {{2, 2, 2}}, {{-40, 0, 0}}},
      {"LeaveXhi", "free", {{30, 30, 30}}, {{2, 2, 2}}, {{40, 0, 0}}},
      {"LeaveYlo", "free", {{30, 30, 30}}, {{2, 2, 2}}, {{0, -40, 0}}},
      {"LeaveYhi", "free", {{30, 30, 30}}, {{2, 2, 2}}, {{3, 40, 0}}},
      {"LeaveZlo", "free", {{30, 30, 30}}, {{2, 2, 2}}, {{0, 0, -40}}},
      {"LeaveZhi", "free", {{30, 30, 30}}, {{2, 2, 2}}, {{0, -5, 40}}},
      {"Outside", "free", {{-10, -10, -10}}, {{2, 2, 2}}, {{3, 0, 0}}},
      {"UnseenBeforeObstacle", "gap", {{10, 3, 3}}, {{1, 1, 1}}, {{40, 0, 0}}},
      {"BlockedAtStart", "a", {{9, 9, 9}}, {{2, 2, 2}}, {{5, 5, 5}}},
      {"LimitLow", "d", {{-lim, 5, 5}}, {{1, 1, 1}}, {{2 * lim - 1, 0, 0}}},
      {"LimitHigh", "d", {{lim - 1, 5, 5}}, {{1, 1, 1}}, {{-2 * lim + 1, 0, 0}}},
      {"BeyondLimitSide", "d", {{lim - 1, 5, 5}}, {{2, 1, 1}}, {{0, 0, 0}}},
      {"BeyondLimitMove", "d", {{-lim, 5, 5}}, {{1, 1, 1}}, {{2 * lim, 0, 0}}},
      {"BeyondLimitLo", "d", {{-lim - 1, 5, 5}}, {{1, 1, 1}}, {{0, 0, 0}}},
      {"ZeroSide", "d", {{5, 5, 5}}, {{1, 0, 1}}, {{1, 1, 1}}},
  };
  for (const Case& c : cases) {
    const Map& m = *maps[c.map];
    motion_result r[2];
    for (int s = 0; s < 2; ++s)
      if (!same(m, c.lo, c.side, c.d, kTest, s ? collision_status::unseen : collision_status::occupied, &r[s])) {
        std::fprintf(stderr, "%s: traversal and brute force differ (stop_at %d)\n", c.name.c_str(), s);
        return 1;
      }
    if (r[0].valid && c.d(0) == 0 && c.d(1) == 0 && c.d(2) == 0 && (int)r[0].status != strict_brute(m, c.lo, c.side)) {
      std::fprintf(stderr, "%s: d = 0 differs from the strict box\n", c.name.c_str());
      return 1;
    }
    std::printf("%s %d %d %lld %lld %d %lld %lld\n", c.name.c_str(), r[0].valid ? 1 : 0, r[0].valid ? (int)r[0].status : 255, (long long)r[0].t_first.num,
                (long long)r[0].t_first.den, r[1].valid ? (int)r[1].status : 255, (long long)r[1].t_first.num, (long long)r[1].t_first.den);
  }
  return 0;
}

template <typename T>
static void random_map(std::mt19937& rng, int t, long* checked, long* bad) {
  typedef typename voxel_traits<T>::value_type V;
  const se::geometry::voxel_test<T> test = {5.f, false};
  const int size = 64;
  Builder<T> b(size);
  const int nb = 1 + (int)(rng() % 40);
  for (int i = 0; i < nb; ++i) b.allocate((int)(rng() % (size / 2)) + ((t & 2) ? 0 : size / 4), (int)(rng() % (size / 2)), (int)(rng() % size));
  auto m = b.build();
  const V init = voxel_traits<T>::initValue();
  auto value = [&](unsigned r) { V v = init; if (r == 1) { v.x = 2.f; v.y = 1; } else if (r == 2) { v.x = 10.f; v.y = 1; } return v; };   // 0 unseen
  for (auto& bl : m->getBlockBuffer())
    for (int v = 0; v < 512; ++v) { const int r = (int)(rng() % 64); bl->voxel_block_[v] = value(r == 0 ? 1 : (r < 8 ? 0 : 2)); }
  for (auto& nd : m->getNodesBuffer())
    for (int v = 0; v < 8; ++v) nd->value_[v] = value(rng() % 8 == 0 ? 1 : (rng() % 2 ? 0 : 2));
  for (int k = 0; k < 400; ++k) {
    int3 lo, side, d;
    const int kind = k % 8;   // 0: d = 0, 1: axis-aligned, 2: planar, else general
    const int axis = (int)(rng() % 3);
    for (int a = 0; a < 3; ++a) {
      side(a) = 1 + (int)(rng() % 12);
      lo(a) = (int)(rng() % (unsigned)(size + 40)) - 24;
      d(a) = (int)(rng() % 141) - 70;
      if (kind == 0 || (kind == 1 && a != axis) || (kind == 2 && a == axis)) d(a) = 0;
    }
    const collision_status stop = (k / 8) % 2 ? collision_status::unseen : collision_status::occupied;
    ++*checked;
    if (!same(*m, lo, side, d, test, stop, nullptr)) {
      if (*bad < 5) std::fprintf(stderr, "map %d motion (%d %d %d | %d %d %d | %d %d %d) stop_at %d: traversal and brute force differ\n", t, lo(0), lo(1), lo(2),
                                 side(0), side(1), side(2), d(0), d(1), d(2), (int)stop);
      ++*bad;
    }
  }
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "kats";
  if (mode == "kats") return run_kats();
  if (mode == "random") {
    const int n = argc > 2 ? std::atoi(argv[2]) : 4;
    std::mt19937 rng(argc > 3 ? (unsigned)std::atoi(argv[3]) : 1u);
    long checked = 0, bad = 0;
    for (int t = 0; t < n; ++t) {
      if (t % 2) random_map<OFusion>(rng, t, &checked, &bad);
      else random_map<SDF>(rng, t, &checked, &bad);
    }
    std::printf("checked %ld mismatches %ld\n", checked, bad);
    return bad ? 1 : 0;
  }
  return 2;
}
