/*
 * Known-answer and randomised tests of the oriented box collision queries on the host mirror (include/se/oriented_collision.hpp): the
 * recursive traversal against the literal definition (every voxel of the box's bounding box).
 *
 *   oriented_kats kats               the hand-worked cases of tests/oriented_util.py on 64^3 SDF maps; one line per case:
 *                                    "<name> <status>" (0 occupied, 1 unseen, 2 empty, 255 invalid).  A case whose traversal and brute force
 *                                    differ ends the program with 1 (the Limit* cases, whose bounding boxes are too large, run the traversal only).
 *   oriented_kats random <n> <seed>  n random 64^3 maps (both fields in turn) x 400 boxes; prints "checked <k> mismatches <m> occupied <n> unseen <n> empty <n> invalid <n>"
 *                                    (the traversal's answers)
 *   oriented_kats pairs              reads "c h0 h1 h2 v s" (12 + 3 + 1 integers) per line from stdin, prints the predicate (0 / 1) per line
 *
 * Values: x = 10 empty, x = 2 occupied, initValue() unseen, judged by voxel_test{5, below} (as tests/cpp/motion_kats.cpp).
 */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "se/octree.hpp"
#include "se/octree_collision.hpp"
#include "se/oriented_collision.hpp"

using se::geometry::collision_status;
using se::geometry::int3;
using se::geometry::oriented_box;
using se::geometry::oriented_result;

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
  void allocate(int x, int y, int z, int to_level = 0) {
    const int leaf = log2i(size) - 3;
    const int last = to_level ? to_level : leaf;
    for (int l = 1; l <= last; ++l) {
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

/* nothing but the level-2 octant [32, 48)^3, a node without children; its value_ and its own slot in its parent occupied */
static std::unique_ptr<Map> octant_map() {
  Builder<SDF> b(64);
  b.allocate(32, 32, 32, 2);
  auto m = b.build();
  for (auto& nd : m->getNodesBuffer()) {
    if (nd->side_ == 16)
      for (int v = 0; v < 8; ++v) nd->value_[v].x = 2.f;
    if (nd->side_ == 32) nd->value_[0].x = 2.f;
  }
  return m;
}

struct Case { const char* name; const char* map; int32_t b[12]; };

template <typename T, typename TestF>
static bool same(const se::Octree<T>& m, const oriented_box& b, TestF test, oriented_result* out) {
  const oriented_result a = se::geometry::oriented_status(m, b, test);
  const oriented_result d = se::geometry::oriented_status_brute(m, b, test);
  if (out) *out = a;
  if (a.valid != d.valid) return false;
  return !a.valid || a.status == d.status;
}

static int run_kats() {
  std::map<std::string, std::unique_ptr<Map>> maps;
  maps["a"] = free_map({{{10, 10, 10}}});
  maps["free"] = free_map({});
  maps["octant"] = octant_map();
  const int CL = se::geometry::oriented_centre_limit, HL = se::geometry::oriented_axis_limit;
  const int32_t MIN = INT32_MIN;
  const Case cases[] = {
      {"DiamondMissesCorner", "a", {112, 112, 168, 32, 32, 0, -32, 32, 0, 0, 0, 4}},
      {"DiamondVertexOnCorner", "a", {96, 160, 168, 32, 32, 0, -32, 32, 0, 0, 0, 4}},
      {"DiamondVertexInside", "a", {97, 160, 168, 32, 32, 0, -32, 32, 0, 0, 0, 4}},
      {"FaceSlides", "a", {144, 168, 168, 16, 0, 0, 0, 8, 6, 0, -6, 8}},
      {"FaceSlidesIn", "a", {145, 168, 168, 16, 0, 0, 0, 8, 6, 0, -6, 8}},
      {"ThinPlate", "a", {168, 168, 168, 8, 8, 0, 1, 0, 0, 0, 0, 4}},
      {"InsideVoxel", "a", {168, 168, 168, 4, 3, 0, -3, 4, 0, 0, 0, 5}},
      {"InsideNext", "a", {184, 168, 168, 4, 3, 0, -3, 4, 0, 0, 0, 5}},
      {"PartlyOutside", "free", {8, 168, 168, 8, 6, 0, -6, 8, 0, 0, 0, 10}},
      {"WhollyOutside", "free", {-100, 168, 168, 8, 6, 0, -6, 8, 0, 0, 0, 10}},
      {"OctantValue", "octant", {640, 640, 640, 40, 30, 0, -30, 40, 0, 0, 0, 50}},
      {"OctantUnseen", "octant", {160, 160, 160, 40, 30, 0, -30, 40, 0, 0, 0, 50}},
      {"SkewMisses", "a", {192, 160, 168, 16, 0, 0, 16, 16, 0, 0, 0, 8}},
      {"SkewTouches", "a", {191, 160, 168, 16, 0, 0, 16, 16, 0, 0, 0, 8}},
      {"InvalidDet", "a", {168, 168, 168, 8, 8, 0, 1, 0, 0, 8, 8, 0}},
      {"InvalidDetZeroAxis", "a", {168, 168, 168, 8, 8, 0, 0, 0, 0, 0, 0, 4}},
      {"InvalidCentre", "a", {CL + 1, 168, 168, 4, 3, 0, -3, 4, 0, 0, 0, 5}},
      {"InvalidCentreLow", "a", {168, -CL - 1, 168, 4, 3, 0, -3, 4, 0, 0, 0, 5}},
      {"InvalidAxis", "a", {168, 168, 168, HL + 1, 0, 0, 0, 8, 0, 0, 0, 8}},
      {"InvalidAxisLow", "a", {168, 168, 168, 8, 0, 0, 0, 8, 0, 0, 0, -HL - 1}},
      {"InvalidInt32MinCentre", "a", {MIN, 168, 168, 4, 3, 0, -3, 4, 0, 0, 0, 5}},
      {"InvalidInt32MinAxis", "a", {168, 168, 168, MIN, MIN, MIN, 0, MIN, 0, 0, 0, MIN}},
      {"LimitCentreHigh", "a", {CL, CL, CL, 4, 3, 0, -3, 4, 0, 0, 0, 5}},
      {"LimitCentreLow", "a", {-CL, 168, 168, 4, 3, 0, -3, 4, 0, 0, 0, 5}},
      {"LimitAxesFree", "free", {512, 512, 512, HL, 0, 0, 0, HL, 0, 0, 0, HL}},
      {"LimitAxesOccupied", "a", {512, 512, 512, 0, HL, 0, -HL, 0, 0, 0, 0, -HL}},
  };
  for (const Case& c : cases) {
    const Map& m = *maps[c.map];
    const oriented_box b = se::geometry::oriented_box_from(c.b);
    oriented_result r;
    if (std::string(c.name).compare(0, 5, "Limit") == 0) {
      r = se::geometry::oriented_status(m, b, kTest);
    } else if (!same(m, b, kTest, &r)) {
      std::fprintf(stderr, "%s: traversal and brute force differ\n", c.name);
      return 1;
    }
    std::printf("%s %d\n", c.name, r.valid ? (int)r.status : 255);
  }
  return 0;
}

template <typename T>
static void random_map(std::mt19937& rng, int t, long* checked, long* bad, long* seen) {
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
  std::uniform_real_distribution<double> uni(0.0, 1.0);
  std::normal_distribution<double> normal(0.0, 1.0);
  const int sub = se::geometry::oriented_sub;
  for (int k = 0; k < 400; ++k) {
    oriented_box bx;
    const int kind = k % 8;   // 0: axis-aligned on voxel boundaries, 1: axis-aligned anywhere, 2: skew, else rotated
    for (int a = 0; a < 3; ++a) bx.c[a] = (int)(rng() % (unsigned)((size + 16) * sub)) - 8 * sub;
    double len[3];
    for (int a = 0; a < 3; ++a) len[a] = std::exp(uni(rng) * std::log(6.0 * sub));   // 1 / 16 voxel .. 6 voxels
    if (kind <= 1) {
      for (int i = 0; i < 3; ++i)
        for (int a = 0; a < 3; ++a) bx.h[i][a] = i == a ? (kind == 0 ? (sub / 2) * (1 + (int)(rng() % 10)) : 1 + (int)len[i]) : 0;
      if (kind == 0)
        for (int a = 0; a < 3; ++a) bx.c[a] = (bx.c[a] / sub) * sub + (bx.h[a][a] % sub);
    } else {
      double q[4], nrm = 0;
      for (int a = 0; a < 4; ++a) { q[a] = normal(rng); nrm += q[a] * q[a]; }
      nrm = std::sqrt(nrm);
      const double w = q[0] / nrm, x = q[1] / nrm, y = q[2] / nrm, z = q[3] / nrm;
      const double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)},
                              {2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)},
                              {2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
      for (int i = 0; i < 3; ++i)
        for (int a = 0; a < 3; ++a) bx.h[i][a] = (int)std::nearbyint(R[a][i] * len[i] + (kind == 2 && i == 1 ? 0.5 * R[a][0] * len[0] : 0.0));
    }
    ++*checked;   // (a box whose rounded axes are dependent is invalid: both sides must say so)
    oriented_result r;
    const bool ok = same(*m, bx, test, &r);
    ++seen[r.valid ? (int)r.status : 3];
    if (!ok) {
      if (*bad < 5) {
        std::fprintf(stderr, "map %d box (", t);
        for (int a = 0; a < 3; ++a) std::fprintf(stderr, "%d ", bx.c[a]);
        for (int i = 0; i < 3; ++i)
          for (int a = 0; a < 3; ++a) std::fprintf(stderr, "%d ", bx.h[i][a]);
        std::fprintf(stderr, "): traversal and brute force differ\n");
      }
      ++*bad;
    }
  }
}

static int run_pairs() {
  long long v[16];
  for (;;) {
    for (int i = 0; i < 16; ++i)
      if (std::scanf("%lld", &v[i]) != 1) return 0;
    int32_t b[12];
    for (int i = 0; i < 12; ++i) b[i] = (int32_t)v[i];
    std::printf("%d\n", se::geometry::oriented_touched(se::geometry::oriented_box_from(b), (int)v[12], (int)v[13], (int)v[14], (int)v[15]) ? 1 : 0);
  }
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "kats";
  if (mode == "kats") return run_kats();
  if (mode == "pairs") return run_pairs();
  if (mode == "random") {
    const int n = argc > 2 ? std::atoi(argv[2]) : 4;
    std::mt19937 rng(argc > 3 ? (unsigned)std::atoi(argv[3]) : 1u);
    long checked = 0, bad = 0, seen[4] = {0, 0, 0, 0};
    for (int t = 0; t < n; ++t) {
      if (t % 2) random_map<OFusion>(rng, t, &checked, &bad, seen);
      else random_map<SDF>(rng, t, &checked, &bad, seen);
    }
    std::printf("checked %ld mismatches %ld occupied %ld unseen %ld empty %ld invalid %ld\n", checked, bad, seen[0], seen[1], seen[2], seen[3]);
    return bad ? 1 : 0;
  }
  return 2;
}
