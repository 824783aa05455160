/*
 * Known-answer and randomised tests of the distance field on the host mirror (include/se/distance_field.hpp): the literal definition (a),
 * the three-pass restatement (b) that the device follows, and the clearance traversal of include/se/clearance.hpp asked once per voxel,
 * held equal voxel by voxel in d2 and in the nearest voxel.
 *
 *   field_kats kats                 hand-worked requests on 64^3 SDF maps (those of tests/cpp/clearance_kats.cpp); one line per voxel of the
 *                                   region, in (z, y, x) order: "<name> <d2, stop_at occupied> <x> <y> <z> <d2, stop_at unseen> <x> <y> <z>"
 *                                   (d2 -1 = nothing within r_max; then x y z are INT32_MIN; an invalid request prints "<name> invalid").  A
 *                                   request on which (a), (b) and the traversal differ ends the program with 1.
 *   field_kats random <n> <seed>    n random 64^3 maps (both fields in turn, node-only octants included) x 50 requests (region sides 1 .. 5,
 *                                   robot sides 1 .. 3, r_max 0 .. 6, now and then 20; regions reach outside the volume); prints
 *                                   "sdf <requests> ofusion <requests> voxels <v> none <k> mismatches <m> ties <t>" (ties: voxels whose d2 a
 *                                   second blocking voxel attains as well -- the tie-break was exercised)
 *
 * Values: x = 10 empty, x = 2 occupied, initValue() unseen, judged by voxel_test{5, below}.
 *
 * The hand requests (lo, side | robot | r_max); the first six are cases of clearance_kats.cpp asked as one-voxel regions:
 *   CornerR15 / CornerR16   a, (0,0,0) 1 | 1 | 15, 16: the occupied voxel (10,10,10) is 9 away on every axis, d2 243: beyond 15, within 16.
 *                           Unseen: the voxels at -1 touch the box: d2 0 at (-1,-1,-1).
 *   WallTie                 wall (the plane x = 20), (10,5,5) 1 | 2 | 10: gap 20 - 12 = 8, d2 64, attained by y, z in [4,7]: (20,4,4).
 *                           Unseen: the faces y = 0 and z = 0 are 5 away: (9,-1,4) and (9,4,-1); z first.
 *   FreeR30 / FreeR29       free, (30,30,30) 1 | 2 | 30, 29: the low faces are 30 away: unseen 900 at (29,29,-1); nothing with 29.
 *   GapBox                  gap, (10,3,3) 1 | 1 | 32: occupied (40,3,3) at 29: 841.  Unseen: the faces y = 0, z = 0 at 3: 9 at (9,2,-1).
 *   OctantCorner            octant, (20,22,25) 1 | 2 | 14: gaps 10, 8, 5 to the node-only octant: 189 at (32,32,32); unseen 0 at (19,21,24).
 *   RowAway                 a, (12,10,10) (3,1,1) | 1 | 3: the voxels x = 12, 13, 14 are 1, 2, 3 away from (10,10,10): d2 1, 4, 9, each at
 *                           (10,10,10); the volume's faces are 10 away, so unseen changes nothing.
 *   RowRobot                a, (5,10,10) (4,1,1) | (3,1,1) | 2: the boxes [x, x + 3) for x = 5 .. 8: gaps 2, 1, 0, 0: d2 4, 1, 0, 0.
 *   RMax256 / ZeroRobot / Robot257 / BeyondLimit   invalid.
 */
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "se/clearance.hpp"
#include "se/distance_field.hpp"
#include "se/octree.hpp"
#include "se/octree_collision.hpp"

using se::geometry::clearance_result;
using se::geometry::collision_status;
using se::geometry::field_request;
using se::geometry::field_result;
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

struct Tally { long voxels = 0, none = 0, bad = 0, ties = 0; };

/* (a) == (b) == the clearance traversal per voxel; `out` receives (b).  Counts the voxels, those without an answer, the mismatches and
 * (count_ties) the voxels whose d2 a second blocking voxel attains. */
template <typename T, typename TestF>
static bool same(const se::Octree<T>& m, const field_request& q, TestF test, collision_status stop, field_result* out, Tally* tally, bool count_ties) {
  field_result a, b;
  const bool va = se::geometry::distance_field_brute(m, q, test, stop, a), vb = se::geometry::distance_field(m, q, test, stop, b);
  if (out) *out = b;
  if (va != vb) { ++tally->bad; return false; }
  if (!va) return true;
  bool ok = a.d2.size() == b.d2.size() && a.nearest.size() == b.nearest.size();
  size_t at = 0;
  for (int k = 0; ok && k < q.side(2); ++k)
    for (int j = 0; j < q.side(1); ++j)
      for (int i = 0; i < q.side(0); ++i, ++at) {
        const int3 v = {{q.lo(0) + i, q.lo(1) + j, q.lo(2) + k}};
        const clearance_result c = se::geometry::clearance(m, v, q.robot, q.r_max, test, stop);
        bool eq = (int64_t)a.d2[at] == c.d2 && (int64_t)b.d2[at] == c.d2;
        for (int x = 0; x < 3; ++x) eq = eq && a.nearest[3 * at + x] == c.nearest(x) && b.nearest[3 * at + x] == c.nearest(x);
        ++tally->voxels;
        tally->none += c.d2 < 0;
        if (!eq) { ++tally->bad; ok = false; }
        if (count_ties && c.d2 >= 0) {
          int count = 0;
          const int r = q.r_max + 1;
          for (int z = v(2) - r; z < v(2) + q.robot(2) + r && count < 2; ++z)
            for (int y = v(1) - r; y < v(1) + q.robot(1) + r && count < 2; ++y)
              for (int x = v(0) - r; x < v(0) + q.robot(0) + r && count < 2; ++x) {
                const int3 w = {{x, y, z}};
                if (se::geometry::cube_d2(v, q.robot, w, 1) == c.d2 && se::geometry::field_detail::blocks(m, x, y, z, test, stop)) ++count;
              }
          tally->ties += count > 1;
        }
      }
  return ok;
}

struct Case { std::string name, map; field_request q; };

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
      {"CornerR15", "a", {{{0, 0, 0}}, {{1, 1, 1}}, {{1, 1, 1}}, 15}},
      {"CornerR16", "a", {{{0, 0, 0}}, {{1, 1, 1}}, {{1, 1, 1}}, 16}},
      {"WallTie", "wall", {{{10, 5, 5}}, {{1, 1, 1}}, {{2, 2, 2}}, 10}},
      {"FreeR30", "free", {{{30, 30, 30}}, {{1, 1, 1}}, {{2, 2, 2}}, 30}},
      {"FreeR29", "free", {{{30, 30, 30}}, {{1, 1, 1}}, {{2, 2, 2}}, 29}},
      {"GapBox", "gap", {{{10, 3, 3}}, {{1, 1, 1}}, {{1, 1, 1}}, 32}},
      {"OctantCorner", "octant", {{{20, 22, 25}}, {{1, 1, 1}}, {{2, 2, 2}}, 14}},
      {"RowAway", "a", {{{12, 10, 10}}, {{3, 1, 1}}, {{1, 1, 1}}, 3}},
      {"RowRobot", "a", {{{5, 10, 10}}, {{4, 1, 1}}, {{3, 1, 1}}, 2}},
      {"RMax256", "a", {{{0, 0, 0}}, {{1, 1, 1}}, {{1, 1, 1}}, 256}},
      {"ZeroRobot", "a", {{{0, 0, 0}}, {{1, 1, 1}}, {{1, 0, 1}}, 4}},
      {"Robot257", "a", {{{0, 0, 0}}, {{1, 1, 1}}, {{257, 1, 1}}, 4}},
      {"BeyondLimit", "a", {{{lim - 2, 0, 0}}, {{1, 1, 1}}, {{2, 1, 1}}, 4}},
  };
  for (const Case& c : cases) {
    const Map& m = *maps[c.map];
    if (!se::geometry::field_valid(c.q)) {
      field_result r;
      if (se::geometry::distance_field(m, c.q, kTest, collision_status::occupied, r) || se::geometry::distance_field_brute(m, c.q, kTest, collision_status::occupied, r)) return 1;
      std::printf("%s invalid\n", c.name.c_str());
      continue;
    }
    field_result r[2];
    Tally t;
    for (int s = 0; s < 2; ++s)
      if (!same(m, c.q, kTest, s ? collision_status::unseen : collision_status::occupied, &r[s], &t, false)) {
        std::fprintf(stderr, "%s: the definition, the three passes and the traversal differ (stop_at %d)\n", c.name.c_str(), s);
        return 1;
      }
    for (size_t at = 0; at < r[0].d2.size(); ++at)
      std::printf("%s %d %d %d %d %d %d %d %d\n", c.name.c_str(), r[0].d2[at], r[0].nearest[3 * at], r[0].nearest[3 * at + 1], r[0].nearest[3 * at + 2], r[1].d2[at],
                  r[1].nearest[3 * at], r[1].nearest[3 * at + 1], r[1].nearest[3 * at + 2]);
  }
  return 0;
}

template <typename T>
static void random_map(std::mt19937& rng, int t, long* requests, Tally* tally) {
  typedef typename voxel_traits<T>::value_type V;
  const se::geometry::voxel_test<T> test = {5.f, false};
  const int size = 64;
  Builder<T> b(size);
  const int nb = 1 + (int)(rng() % 40);
  for (int i = 0; i < nb; ++i) b.allocate((int)(rng() % (size / 2)) + ((t & 2) ? 0 : size / 4), (int)(rng() % (size / 2)), (int)(rng() % size));
  // node-only octants: levels above the leaf level without children
  for (int i = 0; i < 3; ++i) b.allocate((int)(rng() % size), (int)(rng() % size), (int)(rng() % size), 1 + (int)(rng() % 2));
  auto m = b.build();
  const V init = voxel_traits<T>::initValue();
  auto value = [&](unsigned r) { V v = init; if (r == 1) { v.x = 2.f; v.y = 1; } else if (r == 2) { v.x = 10.f; v.y = 1; } return v; };   // 0 unseen
  // sparse obstacles, so that the answers spread over many distances; maps 4k + 3 are denser
  const int rare = (t & 3) == 3 ? 16 : 400;
  for (auto& bl : m->getBlockBuffer())
    for (int v = 0; v < 512; ++v) { const int r = (int)(rng() % rare); bl->voxel_block_[v] = value(r == 0 ? 1 : (r < rare / 8 ? 0 : 2)); }
  for (auto& nd : m->getNodesBuffer())
    for (int v = 0; v < 8; ++v) nd->value_[v] = value(rng() % 6 == 0 ? 1 : (rng() % 4 ? 2 : 0));
  for (int k = 0; k < 50; ++k) {
    field_request q;
    for (int a = 0; a < 3; ++a) {
      q.side(a) = 1 + (int)(rng() % 5);
      q.robot(a) = 1 + (int)(rng() % 3);
      q.lo(a) = (int)(rng() % (unsigned)(size + 28)) - 16;
    }
    q.r_max = k % 25 == 0 ? 20 : (int)(rng() % 7);
    const collision_status stop = (k / 4) % 2 ? collision_status::unseen : collision_status::occupied;
    ++*requests;
    const long before = tally->bad;
    if (!same(*m, q, test, stop, nullptr, tally, q.r_max <= 6) && before < 5)
      std::fprintf(stderr, "map %d request (%d %d %d | %d %d %d | %d %d %d | %d) stop_at %d: the definition, the three passes and the traversal differ\n", t, q.lo(0),
                   q.lo(1), q.lo(2), q.side(0), q.side(1), q.side(2), q.robot(0), q.robot(1), q.robot(2), q.r_max, (int)stop);
  }
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "kats";
  if (mode == "kats") return run_kats();
  if (mode == "random") {
    const int n = argc > 2 ? std::atoi(argv[2]) : 4;
    std::mt19937 rng(argc > 3 ? (unsigned)std::atoi(argv[3]) : 1u);
    long requests[2] = {0, 0};
    Tally tally;
    for (int t = 0; t < n; ++t) {
      if (t % 2) random_map<OFusion>(rng, t, &requests[1], &tally);
      else random_map<SDF>(rng, t, &requests[0], &tally);
    }
    std::printf("sdf %ld ofusion %ld voxels %ld none %ld mismatches %ld ties %ld\n", requests[0], requests[1], tally.voxels, tally.none, tally.bad, tally.ties);
    return tally.bad ? 1 : 0;
  }
  return 2;
}
