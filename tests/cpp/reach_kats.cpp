/*
 * Known-answer and randomised tests of the reachability field on the host mirror (include/se/reach_field.hpp): the literal definition (a), a
 * queue BFS on keys, and the restatement (b) of the device's tile scheme under every tile order, with current and with stale halos, with the
 * device's tile and with a small one, held equal position by position in steps, seed and next, with the round bound rounds <= max steps + 2
 * asserted for every run of (b).
 *
 *   reach_kats kats                 hand-worked requests on 64^3 SDF maps (those of tests/cpp/field_kats.cpp); one line per position of the
 *                                   region, in (z, y, x) order: "<name> <steps seed next, stop_at occupied> <steps seed next, stop_at unseen>"
 *                                   (steps -1 = not free or cut off; then seed and next are 255; next 6 = at a seed; an invalid request
 *                                   prints "<name> invalid").  A request on which (a) and any run of (b) differ, or on which a run of (b)
 *                                   exceeds the round bound, ends the program with 1.
 *   reach_kats random <n> <seed>    n random 64^3 maps (both fields in turn, node-only octants included) x 50 requests (region sides 1 .. 12,
 *                                   robot sides 1 .. 3, 1 .. 5 seeds in and around the region, duplicates among them; regions reach outside
 *                                   the volume); prints "sdf <requests> ofusion <requests> positions <p> free <f> reached <r> cut <c>
 *                                   runs <b> mismatches <m> late <l> most_rounds <k>" (cut: free, yet cut off from every seed; runs: runs of
 *                                   (b); late: runs beyond the round bound)
 *
 * Values: x = 10 empty, x = 2 occupied, initValue() unseen, judged by voxel_test{5, below}.
 *
 * The hand requests (lo, side | robot | seeds), answers as steps/seed/next per position:
 *   RowSplit    a, (8,10,10) (5,1,1) | 1 | (8,10,10) (12,10,10): a row of five through the occupied voxel (10,10,10).  Seed 0 holds x = 8 and
 *               reaches 9 (one move, -x: code 0); 10 is not free; seed 1 holds 12 and reaches 11 (+x: code 1).  0/0/6 1/0/0 -1 1/1/1 0/1/6.
 *   RowTie      free, (30,30,30) (5,1,1) | 1 | (30,30,30) (34,30,30): a free row, seeds at both ends.  The middle is two moves from either:
 *               the lower index wins, key 2 * 256 + 0, and its -x neighbour holds 256 + 0.  0/0/6 1/0/0 2/0/0 1/1/1 0/1/6.
 *   SquareNext  free, (30,30,30) (2,2,1) | 1 | (30,30,30) twice and (29,30,30): the duplicate resolves to index 0, the third seed lies
 *               outside.  (31,30) goes -x, (30,31) goes -y (code 2), (31,31) may go -x or -y: the lower code.  0/0/6 1/0/0 1/0/2 2/0/0.
 *   RobotTwo    a, (7,10,10) (5,1,1) | (2,1,1) | (9,10,10) (11,10,10): the boxes at 9 and 10 hold (10,10,10), so the seed at 9 is ignored and
 *               7, 8 -- free -- are cut off from the seed at 11.  -1 -1 -1 -1 0/1/6.
 *   WallCut     wall (the plane x = 20), (18,5,5) (5,1,1) | 1 | (18,5,5): 18, 19 reached, the wall and what lies behind it not.
 *   AcrossFace  free, (-2,5,5) (4,1,1) | 1 | (1,5,5): x = -2, -1 lie outside the volume, unseen: free with stop_at occupied (3/0/1 2/0/1
 *               1/0/1 0/0/6), not free with stop_at unseen (-1 -1 1/0/1 0/0/6).
 *   NoSeed      a, (10,10,10) (2,1,1) | 1 | (10,10,10) and (INT32_MAX, INT32_MIN, 0): one seed on the occupied voxel, one far outside:
 *               nothing is reached.
 *   ZeroRobot / Robot257 / BeyondLimit   invalid.
 */
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "se/octree.hpp"
#include "se/octree_collision.hpp"
#include "se/reach_field.hpp"

using se::geometry::collision_status;
using se::geometry::int3;
using se::geometry::reach_order;
using se::geometry::reach_request;
using se::geometry::reach_result;
using se::geometry::reach_schedule;

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

struct Tally { long positions = 0, free = 0, reached = 0, cut = 0, runs = 0, bad = 0, late = 0, most_rounds = 0; };

static bool equal(const reach_result& a, const reach_result& b) {
  return a.steps == b.steps && a.seed == b.seed && a.next == b.next && a.counts[0] == b.counts[0] && a.counts[1] == b.counts[1] && a.counts[2] == b.counts[2];
}

/* (a) == every run of (b), and every run within the round bound; `out` receives (a) */
template <typename T, typename TestF>
static bool same(const se::Octree<T>& m, const reach_request& q, TestF test, collision_status stop, reach_result* out, Tally* tally, unsigned shuffle_seed) {
  reach_result a;
  const bool va = se::geometry::reach_field(m, q, test, stop, a);
  if (out) *out = a;
  bool ok = true;
  const int tiles[2][3] = {{32, 8, 8}, {4, 3, 2}};
  const reach_order orders[3] = {reach_order::ascending, reach_order::descending, reach_order::shuffled};
  for (int t = 0; t < 2; ++t)
    for (int o = 0; o < 3; ++o)
      for (int stale = 0; stale < 2; ++stale) {
        reach_schedule sch;
        sch.order = orders[o]; sch.stale_halo = stale != 0; sch.shuffle_seed = shuffle_seed + (unsigned)o;
        for (int k = 0; k < 3; ++k) sch.tile[k] = tiles[t][k];
        reach_result b;
        const bool vb = se::geometry::reach_field_tiled(m, q, test, stop, sch, b);
        ++tally->runs;
        if (va != vb || (va && !equal(a, b))) { ++tally->bad; ok = false; continue; }
        if (!va) continue;
        if (b.counts[3] < 1 || b.counts[3] > a.counts[2] + 2) { ++tally->late; ok = false; }
        if (b.counts[3] > tally->most_rounds) tally->most_rounds = (long)b.counts[3];
      }
  if (va) {
    tally->positions += (long)a.steps.size(); tally->free += (long)a.counts[0]; tally->reached += (long)a.counts[1]; tally->cut += (long)(a.counts[0] - a.counts[1]);
  }
  return ok;
}

struct Case { std::string name, map; reach_request q; };

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
  const int lim = se::geometry::clearance_limit;
  const Case cases[] = {
      {"RowSplit", "a", {{{8, 10, 10}}, {{5, 1, 1}}, {{1, 1, 1}}, {{{8, 10, 10}}, {{12, 10, 10}}}}},
      {"RowTie", "free", {{{30, 30, 30}}, {{5, 1, 1}}, {{1, 1, 1}}, {{{30, 30, 30}}, {{34, 30, 30}}}}},
      {"SquareNext", "free", {{{30, 30, 30}}, {{2, 2, 1}}, {{1, 1, 1}}, {{{30, 30, 30}}, {{30, 30, 30}}, {{29, 30, 30}}}}},
      {"RobotTwo", "a", {{{7, 10, 10}}, {{5, 1, 1}}, {{2, 1, 1}}, {{{9, 10, 10}}, {{11, 10, 10}}}}},
      {"WallCut", "wall", {{{18, 5, 5}}, {{5, 1, 1}}, {{1, 1, 1}}, {{{18, 5, 5}}}}},
      {"AcrossFace", "free", {{{-2, 5, 5}}, {{4, 1, 1}}, {{1, 1, 1}}, {{{1, 5, 5}}}}},
      {"NoSeed", "a", {{{10, 10, 10}}, {{2, 1, 1}}, {{1, 1, 1}}, {{{10, 10, 10}}, {{INT_MAX, INT_MIN, 0}}}}},
      {"ZeroRobot", "a", {{{0, 0, 0}}, {{1, 1, 1}}, {{1, 0, 1}}, {{{0, 0, 0}}}}},
      {"Robot257", "a", {{{0, 0, 0}}, {{1, 1, 1}}, {{257, 1, 1}}, {{{0, 0, 0}}}}},
      {"BeyondLimit", "a", {{{lim - 2, 0, 0}}, {{1, 1, 1}}, {{2, 1, 1}}, {{{0, 0, 0}}}}},
  };
  for (const Case& c : cases) {
    const Map& m = *maps[c.map];
    reach_result r[2];
    Tally t;
    for (int s = 0; s < 2; ++s)
      if (!same(m, c.q, kTest, s ? collision_status::unseen : collision_status::occupied, &r[s], &t, 5u)) {
        std::fprintf(stderr, "%s: the definition and the tile scheme differ, or a run exceeded the round bound (stop_at %d)\n", c.name.c_str(), s);
        return 1;
      }
    if (!se::geometry::reach_valid(c.q)) {
      if (!r[0].steps.empty() || !r[1].steps.empty()) return 1;
      std::printf("%s invalid\n", c.name.c_str());
      continue;
    }
    for (size_t at = 0; at < r[0].steps.size(); ++at)
      std::printf("%s %d %d %d %d %d %d\n", c.name.c_str(), (int)r[0].steps[at], (int)r[0].seed[at], (int)r[0].next[at], (int)r[1].steps[at], (int)r[1].seed[at],
                  (int)r[1].next[at]);
  }
  /* no seed, and more than 255 of them */
  reach_request q = cases[0].q;
  reach_result r;
  q.seeds.clear();
  if (se::geometry::reach_valid(q) || se::geometry::reach_field(*maps["a"], q, kTest, collision_status::occupied, r)) return 1;
  q.seeds.assign(256, {{8, 10, 10}});
  if (se::geometry::reach_valid(q)) return 1;
  q.seeds.assign(255, {{8, 10, 10}});
  if (!se::geometry::reach_valid(q)) return 1;
  return 0;
}

template <typename T>
static void random_map(std::mt19937& rng, int t, long* requests, Tally* tally) {
  typedef typename voxel_traits<T>::value_type V;
  const se::geometry::voxel_test<T> test = {5.f, false};
  const int size = 64;
  Builder<T> b(size);
  const int nb = 1 + (int)(rng() % 60);
  for (int i = 0; i < nb; ++i) b.allocate((int)(rng() % (size / 2)) + ((t & 2) ? 0 : size / 4), (int)(rng() % (size / 2)), (int)(rng() % (size / 2)));
  // node-only octants: levels above the leaf level without children
  for (int i = 0; i < 3; ++i) b.allocate((int)(rng() % size), (int)(rng() % size), (int)(rng() % size), 1 + (int)(rng() % 2));
  auto m = b.build();
  const V init = voxel_traits<T>::initValue();
  auto value = [&](unsigned r) { V v = init; if (r == 1) { v.x = 2.f; v.y = 1; } else if (r == 2) { v.x = 10.f; v.y = 1; } return v; };   // 0 unseen
  // obstacles from sparse to a third of the voxels (where the free space falls apart), now and then an unseen voxel
  static const int kRare[4] = {40, 8, 4, 3};
  const int rare = kRare[(t >> 1) & 3];
  for (auto& bl : m->getBlockBuffer())
    for (int v = 0; v < 512; ++v) { const int r = (int)(rng() % rare); bl->voxel_block_[v] = value(r == 0 ? 1 : (rng() % 50 == 0 ? 0 : 2)); }
  for (auto& nd : m->getNodesBuffer())
    for (int v = 0; v < 8; ++v) nd->value_[v] = value(rng() % 6 == 0 ? 1 : (rng() % 4 ? 2 : 0));
  const auto& blocks = m->getBlockBuffer();
  for (int k = 0; k < 50; ++k) {
    reach_request q;
    // most regions on an allocated block, where the obstacles are; the rest anywhere, outside the volume included
    const int* c = blocks[rng() % blocks.size()]->coordinates();
    for (int a = 0; a < 3; ++a) {
      q.side(a) = 1 + (int)(rng() % 12);
      q.robot(a) = k % 3 ? 1 : 1 + (int)(rng() % 3);
      q.lo(a) = k % 5 ? c[a] + (int)(rng() % 12) - 6 : (int)(rng() % (unsigned)(size + 28)) - 16;
    }
    const int n_seeds = 1 + (int)(rng() % 5);
    for (int s = 0; s < n_seeds; ++s) {
      if (s > 0 && rng() % 6 == 0) { q.seeds.push_back(q.seeds[rng() % q.seeds.size()]); continue; }   // a duplicate
      int3 p;
      for (int a = 0; a < 3; ++a) p(a) = q.lo(a) - 1 + (int)(rng() % (unsigned)(q.side(a) + 2));        // now and then just outside
      q.seeds.push_back(p);
    }
    const collision_status stop = (k / 4) % 2 ? collision_status::unseen : collision_status::occupied;
    ++*requests;
    const long before = tally->bad + tally->late;
    if (!same(*m, q, test, stop, nullptr, tally, (unsigned)(t * 50 + k)) && before < 5)
      std::fprintf(stderr, "map %d request (%d %d %d | %d %d %d | %d %d %d | %zu seeds) stop_at %d: the definition and the tile scheme differ, or a run was late\n", t,
                   q.lo(0), q.lo(1), q.lo(2), q.side(0), q.side(1), q.side(2), q.robot(0), q.robot(1), q.robot(2), q.seeds.size(), (int)stop);
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
    std::printf("sdf %ld ofusion %ld positions %ld free %ld reached %ld cut %ld runs %ld mismatches %ld late %ld most_rounds %ld\n", requests[0], requests[1], tally.positions,
                tally.free, tally.reached, tally.cut, tally.runs, tally.bad, tally.late, tally.most_rounds);
    return tally.bad || tally.late ? 1 : 0;
  }
  return 2;
}
