/*
 * Known-answer and randomised tests of the clearance queries on the host mirror (include/se/clearance.hpp): the recursive pruned traversal
 * against the literal definition (every voxel of the box dilated by r_max + 1), in d2 and in the nearest voxel.
 *
 *   clearance_kats kats               hand-worked cases on 64^3 SDF maps; one line per case:
 *                                     "<name> <d2, stop_at occupied> <x> <y> <z> <d2, stop_at unseen> <x> <y> <z>"
 *                                     (d2 -1 = nothing within r_max, -2 = invalid; then x y z are INT32_MIN).  A case with r_max <= 64 whose
 *                                     traversal and brute force differ ends the program with 1.
 *   clearance_kats random <n> <seed>  n random 64^3 maps (both fields in turn) x 400 queries; prints "sdf <k> ofusion <k> mismatches <m> ties <t>"
 *                                     (ties: answers whose d2 a second blocking voxel attains as well -- the tie-break was exercised)
 *
 * Values: x = 10 empty, x = 2 occupied, initValue() unseen, judged by voxel_test{5, below} (as tests/cpp/motion_kats.cpp).
 *
 * The hand cases (box lo, side; r_max), hi = lo + side:
 *   a: one occupied voxel (10,10,10).
 *     CornerR15 / CornerR16  box (0,0,0) 1: the gap is 10 - 1 = 9 on every axis, d2 = 3 * 81 = 243; 15^2 = 225 < 243 <= 256 = 16^2.  With
 *                            unseen blocking, the voxels at x = -1 (and y, z) touch the box: d2 0, the lowest of them (-1,-1,-1).
 *     CornerR32767           the same with the largest r_max.
 *     Overlap                box (9,9,9) 2 holds the voxel: d2 0 even with r_max 0.
 *     TouchFace / TouchCorner  box (11,10,10) 2 shares the face x = 11 with it, box (11,11,11) 1 only the corner: closed sets, d2 0.
 *     OneAwayR0 / OneAwayR1  box (12,10,10) 1: gap 1; r_max 0 finds nothing, r_max 1 finds it at d2 1.
 *     LimitLow / LimitHigh   lo = -2^19 and hi = 2^19 are valid; far from the voxel; the box is outside the volume, so unseen voxels touch it:
 *                            the lowest is (lo_x - 1, 4, 4).
 *     Beyond* / R32768 / RNegative / ZeroSide   invalid.
 *   wall: the plane x = 20.
 *     WallTie                box (10,5,5) 2: hi_x = 12, gap 8, d2 64, attained by x = 20, y in [4,7], z in [4,7]: the lowest is (20,4,4).
 *                            Unseen: the volume's faces y = 0 and z = 0 are 5 away (25 < 64); the witnesses (9,-1,4) and (9,4,-1); z first.
 *     WallTieAcrossBlocks    box (10,7,7) 2: the tie spans y, z in [6,9], four blocks: (20,6,6).  Unseen: 49, (9,6,-1).
 *   free: nothing occupied.
 *     FreeR30 / FreeR29      box (30,30,30) 2: the low faces are 30 away, the high ones 64 - 32 = 32: d2 900 at (29,29,-1), (29,-1,29),
 *                            (-1,29,29); z first.  r_max 29 finds nothing.
 *   gap: occupied (40,3,3), the block at (24,0,0) unseen.
 *     GapBox                 box (10,3,3) 1, r_max 32: occupied at gap 40 - 11 = 29, d2 841.  Unseen: the faces y = 0, z = 0 at 3 (9)
 *                            beat the unseen block at 24 - 11 = 13 (169): (9,2,-1).
 *   octant: only the level-2 octant [32,48)^3 exists, as a node without children whose eight value_ are occupied (absent octants of side 8).
 *     OctantCorner           box (20,22,25) 2: hi = (22,24,27), gaps 10, 8, 5 to the octant [32,40)^3: d2 189 at its corner (32,32,32).
 *     OctantClamped          box (36,20,50) 2: x overlaps [32,40) and [40,48): the lowest nearest x is lo - 1 = 35; y gap 32 - 22 = 10 at 32;
 *                            z: the box lies above, gap 50 - 48 = 2 at 47: d2 104 at (35,32,47).
 *                            Unseen (both): the box lies in unseen space, d2 0 at (lo - 1).
 */
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "se/clearance.hpp"
#include "se/octree.hpp"
#include "se/octree_collision.hpp"

using se::geometry::clearance_result;
using se::geometry::collision_status;
using se::geometry::int3;

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
  /* the octant of `level` that holds (x, y, z), with its ancestors; the leaf level makes a block */
  void allocate(int x, int y, int z, int level) {
    const int leaf = log2i(size) - 3;
    for (int l = 1; l <= level; ++l) {
      const int side = size >> l;
      const int cx = x & ~(side - 1), cy = y & ~(side - 1), cz = z & ~(side - 1);
      const uint64_t key = morton(cx, cy, cz) | (uint64_t)l;
      if (l < leaf) nodes[key] = side;
      else blocks[key] = {cx, cy, cz};
    }
  }
  void allocate(int x, int y, int z) { allocate(x, y, z, log2i(size) - 3); }
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

struct Case { std::string name, map; int3 lo, side; int r_max; };

template <typename T, typename TestF>
static bool same(const se::Octree<T>& m, const int3& lo, const int3& side, int r_max, TestF test, collision_status stop, clearance_result* out, bool* tie) {
  const clearance_result a = se::geometry::clearance(m, lo, side, r_max, test, stop);
  if (out) *out = a;
  const clearance_result b = se::geometry::clearance_brute(m, lo, side, r_max, test, stop);
  if (tie) {   /* a second blocking voxel at the same distance */
    *tie = false;
    if (a.d2 >= 0) {
      int count = 0;
      const int n = m.size(), r = r_max + 1;
      for (int z = lo(2) - r; z < lo(2) + side(2) + r && count < 2; ++z)
        for (int y = lo(1) - r; y < lo(1) + side(1) + r && count < 2; ++y)
          for (int x = lo(0) - r; x < lo(0) + side(0) + r && count < 2; ++x) {
            const int3 v = {{x, y, z}};
            if (se::geometry::cube_d2(lo, side, v, 1) != a.d2) continue;
            const bool in = x >= 0 && y >= 0 && z >= 0 && x < n && y < n && z < n;
            if ((int)(in ? test(m.get(x, y, z)) : collision_status::unseen) <= (int)stop) ++count;
          }
      *tie = count > 1;
    }
  }
  return a.d2 == b.d2 && a.nearest(0) == b.nearest(0) && a.nearest(1) == b.nearest(1) && a.nearest(2) == b.nearest(2);
}

static int run_kats() {
  std::map<std::string, std::unique_ptr<Map>> maps;
  maps["a"] = free_map({{{10, 10, 10}}});
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
  {   // only the level-2 octant [32, 48)^3, without children, its eight value_ occupied
    Builder<SDF> b(64);
    b.allocate(32, 32, 32, 2);
    maps["octant"] = b.build();
    se::Node<SDF>* n = maps["octant"]->fetch_octant(32, 32, 32, 2);
    if (!n || n->side_ != 16) { std::fprintf(stderr, "octant map: no level-2 node\n"); return 1; }
    for (int v = 0; v < 8; ++v) { n->value_[v].x = 2.f; n->value_[v].y = 1; }
  }
  const int lim = se::geometry::clearance_limit;
  const Case cases[] = {
      {"CornerR15", "a", {{0, 0, 0}}, {{1, 1, 1}}, 15},
      {"CornerR16", "a", {{0, 0, 0}}, {{1, 1, 1}}, 16},
      {"CornerR32767", "a", {{0, 0, 0}}, {{1, 1, 1}}, 32767},
      {"Overlap", "a", {{9, 9, 9}}, {{2, 2, 2}}, 0},
      {"TouchFace", "a", {{11, 10, 10}}, {{2, 2, 2}}, 0},
      {"TouchCorner", "a", {{11, 11, 11}}, {{1, 1, 1}}, 0},
      {"OneAwayR0", "a", {{12, 10, 10}}, {{1, 1, 1}}, 0},
      {"OneAwayR1", "a", {{12, 10, 10}}, {{1, 1, 1}}, 1},
      {"WallTie", "wall", {{10, 5, 5}}, {{2, 2, 2}}, 10},
      {"WallTieAcrossBlocks", "wall", {{10, 7, 7}}, {{2, 2, 2}}, 10},
      {"FreeR30", "free", {{30, 30, 30}}, {{2, 2, 2}}, 30},
      {"FreeR29", "free", {{30, 30, 30}}, {{2, 2, 2}}, 29},
      {"GapBox", "gap", {{10, 3, 3}}, {{1, 1, 1}}, 32},
      {"OctantCorner", "octant", {{20, 22, 25}}, {{2, 2, 2}}, 14},
      {"OctantClamped", "octant", {{36, 20, 50}}, {{2, 2, 2}}, 11},
      {"LimitLow", "a", {{-lim, 5, 5}}, {{1, 1, 1}}, 5},
      {"LimitHigh", "a", {{lim - 1, 5, 5}}, {{1, 1, 1}}, 5},
      {"BeyondLimitLo", "a", {{-lim - 1, 5, 5}}, {{1, 1, 1}}, 5},
      {"BeyondLimitHi", "a", {{lim, 5, 5}}, {{1, 1, 1}}, 5},
      {"R32768", "a", {{0, 0, 0}}, {{1, 1, 1}}, 32768},
      {"RNegative", "a", {{0, 0, 0}}, {{1, 1, 1}}, -1},
      {"ZeroSide", "a", {{5, 5, 5}}, {{1, 0, 1}}, 5},
  };
  for (const Case& c : cases) {
    const Map& m = *maps[c.map];
    clearance_result r[2];
    for (int s = 0; s < 2; ++s) {
      const collision_status stop = s ? collision_status::unseen : collision_status::occupied;
      if (c.r_max > 64 && c.r_max <= se::geometry::clearance_r_max) {   // the brute force would visit 65 536^3 voxels
        r[s] = se::geometry::clearance(m, c.lo, c.side, c.r_max, kTest, stop);
      } else if (!same(m, c.lo, c.side, c.r_max, kTest, stop, &r[s], nullptr)) {
        std::fprintf(stderr, "%s: traversal and brute force differ (stop_at %d)\n", c.name.c_str(), s);
        return 1;
      }
    }
    std::printf("%s %lld %d %d %d %lld %d %d %d\n", c.name.c_str(), (long long)r[0].d2, r[0].nearest(0), r[0].nearest(1), r[0].nearest(2), (long long)r[1].d2,
                r[1].nearest(0), r[1].nearest(1), r[1].nearest(2));
  }
  return 0;
}

template <typename T>
static void random_map(std::mt19937& rng, int t, long* checked, long* bad, long* ties) {
  typedef typename voxel_traits<T>::value_type V;
  const se::geometry::voxel_test<T> test = {5.f, false};
  const int size = 64;
  Builder<T> b(size);
  const int nb = 1 + (int)(rng() % 40);
  for (int i = 0; i < nb; ++i) b.allocate((int)(rng() % (size / 2)) + ((t & 2) ? 0 : size / 4), (int)(rng() % (size / 2)), (int)(rng() % size));
  auto m = b.build();
  const V init = voxel_traits<T>::initValue();
  auto value = [&](unsigned r) { V v = init; if (r == 1) { v.x = 2.f; v.y = 1; } else if (r == 2) { v.x = 10.f; v.y = 1; } return v; };   // 0 unseen
  // sparse obstacles, so that the answers spread over many distances; maps 4k + 3 are denser
  const int rare = (t & 3) == 3 ? 16 : 400;
  for (auto& bl : m->getBlockBuffer())
    for (int v = 0; v < 512; ++v) { const int r = (int)(rng() % rare); bl->voxel_block_[v] = value(r == 0 ? 1 : (r < rare / 8 ? 0 : 2)); }
  for (auto& nd : m->getNodesBuffer())
    for (int v = 0; v < 8; ++v) nd->value_[v] = value(rng() % 6 == 0 ? 1 : (rng() % 4 ? 2 : 0));
  for (int k = 0; k < 400; ++k) {
    int3 lo, side;
    for (int a = 0; a < 3; ++a) {
      side(a) = 1 + (int)(rng() % 6);
      lo(a) = (int)(rng() % (unsigned)(size + 28)) - 16;
    }
    const int r_max = k % 16 == 0 ? 20 : (int)(rng() % 11);
    const collision_status stop = (k / 8) % 2 ? collision_status::unseen : collision_status::occupied;
    ++*checked;
    bool tie = false;
    if (!same(*m, lo, side, r_max, test, stop, nullptr, &tie)) {
      if (*bad < 5) std::fprintf(stderr, "map %d query (%d %d %d | %d %d %d | %d) stop_at %d: traversal and brute force differ\n", t, lo(0), lo(1), lo(2), side(0),
                                 side(1), side(2), r_max, (int)stop);
      ++*bad;
    }
    *ties += tie;
  }
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "kats";
  if (mode == "kats") return run_kats();
  if (mode == "random") {
    const int n = argc > 2 ? std::atoi(argv[2]) : 4;
    std::mt19937 rng(argc > 3 ? (unsigned)std::atoi(argv[3]) : 1u);
    long checked[2] = {0, 0}, bad = 0, ties = 0;
    for (int t = 0; t < n; ++t) {
      if (t % 2) random_map<OFusion>(rng, t, &checked[1], &bad, &ties);
      else random_map<SDF>(rng, t, &checked[0], &bad, &ties);
    }
    std::printf("sdf %ld ofusion %ld mismatches %ld ties %ld\n", checked[0], checked[1], bad, ties);
    return bad ? 1 : 0;
  }
  return 2;
}
