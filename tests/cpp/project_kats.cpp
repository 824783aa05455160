/*
 * Known-answer and randomised tests of the column projections on the host mirror (include/se/project_columns.hpp): the traversal in octant
 * steps against the literal definition (every voxel of every cell through Octree::get), in all four outputs.
 *
 *   project_kats kats                hand-worked cells on the 64^3 SDF map "mix", columns along z; one line per case:
 *                                    "<name> <status first last count, stop_at occupied> <status first last count, stop_at unseen>"
 *                                    (first / last INT32_MIN = no voxel of the cell blocks).  A case whose traversal and literal
 *                                    definition differ ends the program with 1.
 *   project_kats cells <map> <axis> <stop_at> <lo_u> <lo_v> <side_u> <side_v> <a> <b> [<a> <b> ...]
 *                                    the literal definition of one request on the hand map "mix" or "split"; one line per (layer, row):
 *                                    "<l> <j>" and then status first last count of the row's side_u cells.  Ends with 1 if the traversal
 *                                    differs anywhere.
 *   project_kats random <n> <seed>   n random 64^3 maps (both fields in turn) x 24 requests (every axis, both stop_at, 1 .. 16 layers, footprints
 *                                    that stick out); prints "sdf <cells> ofusion <cells> mismatches <m> runs <r>" (runs: cells whose
 *                                    blocking voxels are 16 or more in a row -- longer than two blocks, so an octant step answered)
 *
 * Values: x = 10 empty, x = 2 occupied, initValue() unseen, judged by voxel_test{5, below} (as tests/cpp/clearance_kats.cpp).
 *
 * The hand maps (boxes lo, hi, half open; tests/project_util.py stamps the same on a device map):
 *   mix    blocks [0,32)^3 allocated and empty; occupied: the voxel (10,10,10), the cube [12,15)^3, the bar [3,9) x {20} x [27,29); the block
 *          [24,32) x [0,8) x [0,8) back to initValue() (unseen); the level-2 octant [32,48)^3 a node without children whose eight value_ are
 *          occupied, the level-2 octant [48,64)^3 one whose value_ are empty.  Everything else is absent under initValue(): unseen.
 *   split  blocks [32,64) x [0,32) x [0,32); occupied (40,20,9) and [50,53) x [4,7) x [20,23); unseen block [32,40) x [24,32)^2; occupied
 *          octant [0,16) x [48,64) x [16,32), empty octant [16,32) x [0,16) x [48,64).
 *
 * The hand cells, on mix along z (u = x, v = y), layer [a, b):
 *   OneVoxel              (10,10) [3,13): z = 10 alone.
 *   CubeColumn            (13,13) [0,64): the cube's z = 12 .. 14; above z = 32 nothing is allocated: 32 unseen voxels, so with stop_at
 *                         unseen 3 + 32 = 35 block, the last one z = 63.
 *   FreeColumn            (20,5) [8,16): empty, nothing blocks.
 *   GapColumn             (25,3) [3,13): z = 3 .. 7 lie in the unseen block, z = 8 .. 12 are empty.
 *   OctantOccupied        (40,40) [0,64): z < 32 absent under the root (unseen), [32,48) the occupied octant, [48,64) absent under the
 *                         level-1 node (unseen): 16 occupied, 64 blocking with stop_at unseen.
 *   OctantOccupiedInside  (40,40) [40,56): 8 voxels of the octant, then 8 unseen ones.
 *   OctantEmpty           (50,50) [48,64): the empty octant alone.
 *   OctantEmptyAcross     (50,50) [-9,70): 9 below the volume, 48 unseen inside, 16 empty, 6 above: 63 blocking with stop_at unseen.
 *   Below / Above         (10,10) [-12,-2) and [70,75): outside the volume, unseen, no map access.
 *   OutsideColumn         (-3,10) [3,13): a column outside the volume.
 *   Everything            (10,10) [-2^20, 2^20): 2^20 below, 2^20 - 64 above, z = 10 and the 32 unseen voxels above z = 32.
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
#include "se/project_columns.hpp"

using se::geometry::collision_status;
using se::geometry::project_cell;
using se::geometry::project_request;

static uint64_t spread(uint64_t v) {
  uint64_t r = 0;
  for (int i = 0; i < 21; ++i) r |= ((v >> i) & 1ull) << (3 * i);
  return r;
}
static uint64_t morton(int x, int y, int z) { return spread(x) | (spread(y) << 1) | (spread(z) << 2); }
static int log2i(int s) { int l = 0; while ((1 << l) < s) ++l; return l; }

/* A map under construction: the octants that allocating creates (every ancestor), appended in key order, then linked. */
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
struct Box { int x0, y0, z0, x1, y1, z1; };

static std::unique_ptr<Map> hand_map(const std::vector<Box>& free_boxes, const std::vector<Box>& occupied, const std::vector<Box>& gap, const Box& node_occ,
                                     const Box& node_empty) {
  Builder<SDF> b(64);
  for (const Box& f : free_boxes)
    for (int z = f.z0; z < f.z1; z += 8)
      for (int y = f.y0; y < f.y1; y += 8)
        for (int x = f.x0; x < f.x1; x += 8) b.allocate(x, y, z);
  b.allocate(node_occ.x0, node_occ.y0, node_occ.z0, 2);
  b.allocate(node_empty.x0, node_empty.y0, node_empty.z0, 2);
  auto m = b.build();
  auto set = [&](const Box& r, float x, float y) {
    for (int z = r.z0; z < r.z1; ++z)
      for (int yy = r.y0; yy < r.y1; ++yy)
        for (int xx = r.x0; xx < r.x1; ++xx) {
          se::VoxelBlock<SDF>* bl = m->fetch(xx, yy, z);
          auto& v = bl->voxel_block_[(xx & 7) + 8 * (yy & 7) + 64 * (z & 7)];
          v.x = x; v.y = y;
        }
  };
  const auto init = voxel_traits<SDF>::initValue();
  for (const Box& f : free_boxes) set(f, 10.f, 1);
  for (const Box& o : occupied) set(o, 2.f, 1);
  for (const Box& g : gap) set(g, init.x, init.y);
  const Box* stamped[2] = {&node_occ, &node_empty};
  for (int k = 0; k < 2; ++k) {
    se::Node<SDF>* n = m->fetch_octant(stamped[k]->x0, stamped[k]->y0, stamped[k]->z0, 2);
    if (!n || n->side_ != 16) { std::fprintf(stderr, "hand map: no level-2 node\n"); std::exit(1); }
    for (int v = 0; v < 8; ++v) { n->value_[v].x = k ? 10.f : 2.f; n->value_[v].y = 1; }
  }
  return m;
}

static std::unique_ptr<Map> named_map(const std::string& name) {
  if (name == "mix")
    return hand_map({{0, 0, 0, 32, 32, 32}}, {{10, 10, 10, 11, 11, 11}, {12, 12, 12, 15, 15, 15}, {3, 20, 27, 9, 21, 29}}, {{24, 0, 0, 32, 8, 8}}, {32, 32, 32, 48, 48, 48},
                    {48, 48, 48, 64, 64, 64});
  if (name == "split")
    return hand_map({{32, 0, 0, 64, 32, 32}}, {{40, 20, 9, 41, 21, 10}, {50, 4, 20, 53, 7, 23}}, {{32, 24, 24, 40, 32, 32}}, {0, 48, 16, 16, 64, 32}, {16, 0, 48, 32, 16, 64});
  return nullptr;
}

static bool same(const project_cell& a, const project_cell& b) { return a.status == b.status && a.first == b.first && a.last == b.last && a.count == b.count; }

struct Cell { const char* name; int u, v, a, b; };

static int run_kats() {
  auto m = named_map("mix");
  const int lim = se::geometry::project_limit;
  const Cell cells[] = {
      {"OneVoxel", 10, 10, 3, 13},        {"CubeColumn", 13, 13, 0, 64},         {"FreeColumn", 20, 5, 8, 16},   {"GapColumn", 25, 3, 3, 13},
      {"OctantOccupied", 40, 40, 0, 64},  {"OctantOccupiedInside", 40, 40, 40, 56}, {"OctantEmpty", 50, 50, 48, 64}, {"OctantEmptyAcross", 50, 50, -9, 70},
      {"Below", 10, 10, -12, -2},         {"Above", 10, 10, 70, 75},             {"OutsideColumn", -3, 10, 3, 13}, {"Everything", 10, 10, -lim, lim},
  };
  for (const Cell& c : cells) {
    project_cell r[2];
    for (int s = 0; s < 2; ++s) {
      const collision_status stop = s ? collision_status::unseen : collision_status::occupied;
      r[s] = se::geometry::project_column(*m, 2, c.u, c.v, c.a, c.b, kTest, stop);
      if (!same(r[s], se::geometry::project_column_brute(*m, 2, c.u, c.v, c.a, c.b, kTest, stop))) {
        std::fprintf(stderr, "%s: traversal and literal definition differ (stop_at %d)\n", c.name, s);
        return 1;
      }
    }
    std::printf("%s %d %d %d %d %d %d %d %d\n", c.name, (int)r[0].status, r[0].first, r[0].last, r[0].count, (int)r[1].status, r[1].first, r[1].last, r[1].count);
  }
  return 0;
}

static int run_cells(int argc, char** argv) {
  if (argc < 11 || (argc - 9) % 2) return 2;
  auto m = named_map(argv[2]);
  if (!m) return 2;
  project_request r;
  std::memset(&r, 0, sizeof r);
  r.axis = std::atoi(argv[3]);
  r.stop_at = std::atoi(argv[4]) ? collision_status::unseen : collision_status::occupied;
  r.lo[0] = std::atoi(argv[5]); r.lo[1] = std::atoi(argv[6]); r.side[0] = std::atoi(argv[7]); r.side[1] = std::atoi(argv[8]);
  r.n_layers = (argc - 9) / 2;
  if (r.n_layers > se::geometry::project_max_layers) return 2;
  for (int l = 0; l < r.n_layers; ++l) { r.layers[l][0] = std::atoi(argv[9 + 2 * l]); r.layers[l][1] = std::atoi(argv[10 + 2 * l]); }
  if (!se::geometry::project_valid(r)) return 2;
  const std::vector<project_cell> brute = se::geometry::project_columns_brute(*m, r, kTest), walk = se::geometry::project_columns(*m, r, kTest);
  size_t at = 0;
  bool bad = false;
  for (int l = 0; l < r.n_layers; ++l)
    for (int j = 0; j < r.side[1]; ++j) {
      std::printf("%d %d", l, j);
      for (int i = 0; i < r.side[0]; ++i, ++at) {
        std::printf(" %d %d %d %d", (int)brute[at].status, brute[at].first, brute[at].last, brute[at].count);
        bad = bad || !same(brute[at], walk[at]);
      }
      std::printf("\n");
    }
  if (bad) std::fprintf(stderr, "traversal and literal definition differ\n");
  return bad ? 1 : 0;
}

template <typename T>
static void random_map(std::mt19937& rng, int t, long* checked, long* bad, long* runs) {
  typedef typename voxel_traits<T>::value_type V;
  const se::geometry::voxel_test<T> test = {5.f, false};
  const int size = 64;
  Builder<T> b(size);
  const int nb = 1 + (int)(rng() % 60);
  for (int i = 0; i < nb; ++i) b.allocate((int)(rng() % size), (int)(rng() % size), (int)(rng() % size));
  for (int i = 0; i < 3; ++i) b.allocate((int)(rng() % size), (int)(rng() % size), (int)(rng() % size), 1 + (int)(rng() % 2));   // nodes without children
  auto m = b.build();
  const V init = voxel_traits<T>::initValue();
  auto value = [&](unsigned r) { V v = init; if (r == 1) { v.x = 2.f; v.y = 1; } else if (r == 2) { v.x = 10.f; v.y = 1; } return v; };   // 0 unseen
  const int rare = (t & 3) == 3 ? 6 : 60;
  for (auto& bl : m->getBlockBuffer())
    for (int v = 0; v < 512; ++v) { const int r = (int)(rng() % rare); bl->voxel_block_[v] = value(r == 0 ? 1 : (r < rare / 4 ? 0 : 2)); }
  for (auto& nd : m->getNodesBuffer())
    for (int v = 0; v < 8; ++v) nd->value_[v] = value(rng() % 3);
  for (int k = 0; k < 24; ++k) {
    project_request r;
    std::memset(&r, 0, sizeof r);
    r.axis = k % 3;
    r.stop_at = (k / 3) % 2 ? collision_status::unseen : collision_status::occupied;
    for (int a = 0; a < 2; ++a) {
      r.side[a] = 1 + (int)(rng() % 30);
      r.lo[a] = (int)(rng() % (unsigned)(size + 20)) - 20;
    }
    r.n_layers = k == 0 ? 16 : 1 + (int)(rng() % 4);
    for (int l = 0; l < r.n_layers; ++l) {
      const int a = (int)(rng() % (unsigned)(size + 24)) - 12;
      r.layers[l][0] = a;
      r.layers[l][1] = a + 1 + (int)(rng() % (l % 2 ? 80u : 12u));
    }
    const std::vector<project_cell> brute = se::geometry::project_columns_brute(*m, r, test), walk = se::geometry::project_columns(*m, r, test);
    for (size_t i = 0; i < brute.size(); ++i) {
      ++*checked;
      if (!same(brute[i], walk[i])) {
        if (*bad < 5) std::fprintf(stderr, "map %d request %d cell %zu: traversal and literal definition differ\n", t, k, i);
        ++*bad;
      }
      /* a cell whose blocking voxels are >= 16 in a row was answered (in part) by an octant step */
      if (brute[i].count >= 16 && brute[i].last - brute[i].first + 1 == brute[i].count) ++*runs;
    }
  }
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "kats";
  if (mode == "kats") return run_kats();
  if (mode == "cells") return run_cells(argc, argv);
  if (mode == "random") {
    const int n = argc > 2 ? std::atoi(argv[2]) : 4;
    std::mt19937 rng(argc > 3 ? (unsigned)std::atoi(argv[3]) : 1u);
    long checked[2] = {0, 0}, bad = 0, runs = 0;
    for (int t = 0; t < n; ++t) {
      if (t % 2) random_map<OFusion>(rng, t, &checked[1], &bad, &runs);
      else random_map<SDF>(rng, t, &checked[0], &bad, &runs);
    }
    std::printf("sdf %ld ofusion %ld mismatches %ld runs %ld\n", checked[0], checked[1], bad, runs);
    return bad ? 1 : 0;
  }
  return 2;
}
