/*
 * Known-answer and randomised tests of the segment traces on the host mirror (include/se/segment_trace.hpp): the walk (the three-axis
 * integer DDA with its jumps, what the device does) against the literal definition (every voxel of the segment's bounding box, sorted by
 * entry parameter), in every output.
 *
 *   trace_kats kats               hand-worked cases on 64^3 SDF maps (the maps of tests/cpp/motion_kats.cpp); one line per case:
 *                                 "<name> <valid>" and then, for stop_at occupied and for stop_at unseen,
 *                                 "<status> <num> <den> <first x> <first y> <first z> <unseen> <empty>"
 *                                 (0 occupied, 1 unseen, 2 empty, 255 invalid; num / den in lowest terms, 2 / 1 = free, -1 / 1 = invalid).
 *                                 A case on which the walk without counts differs from the walk with them in status, t_first or first, or
 *                                 a short case on which the walk differs from the literal definition, ends the program with 1.
 *   trace_kats random <n> <seed>  n random 64^3 maps with absent octants (both fields in turn) x 300 short segments of every family;
 *                                 prints "checked <k> mismatches <m>"
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

#include "se/octree.hpp"
#include "se/octree_collision.hpp"
#include "se/segment_trace.hpp"

using se::geometry::collision_status;
using se::geometry::int3;
using se::geometry::trace_result;

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

static bool same(const trace_result& a, const trace_result& b, bool counts) {
  if (a.valid != b.valid) return false;
  if (a.valid && a.status != b.status) return false;
  if (a.t_first.num != b.t_first.num || a.t_first.den != b.t_first.den) return false;
  for (int k = 0; k < 3; ++k)
    if (a.first[k] != b.first[k]) return false;
  return !counts || (a.unseen == b.unseen && a.empty == b.empty);
}

/* walk with counts == walk without counts (but for the counts) and, where asked for, == the literal definition */
template <typename T, typename TestF>
static bool agree(const se::Octree<T>& m, const int32_t seg[6], TestF test, collision_status stop, bool literal, trace_result* out) {
  const trace_result w = se::geometry::trace_walk(m, seg, test, stop, true);
  const trace_result j = se::geometry::trace_walk(m, seg, test, stop, false);
  if (out) *out = w;
  if (!same(w, j, false)) return false;
  return !literal || same(w, se::geometry::trace_literal(m, seg, test, stop), true);
}

struct Case { std::string name, map; int32_t seg[6]; };

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
  const int L = se::geometry::segment_limit;
  const Case cases[] = {
      {"DiagonalCorners", "free", {0, 0, 0, 320, 320, 320}},
      {"DiagonalCornersHit", "a", {0, 0, 0, 320, 320, 320}},
      {"Diagonal3", "a", {8, 8, 8, 328, 328, 328}},
      {"DiagonalTouches", "b", {0, 16, 8, 320, 336, 8}},
      {"DiagonalOpenEnd", "c", {0, 16, 8, 320, 336, 8}},
      {"SlideInWallFace", "wall", {320, 40, 40, 320, 500, 300}},
      {"IntoWall", "wall", {168, 88, 88, 488, 248, 88}},
      {"UnseenGap", "gap", {168, 56, 56, 808, 56, 56}},
      {"LeaveXlo", "free", {488, 488, 488, -152, 488, 488}},
      {"LeaveXhi", "free", {488, 488, 488, 1128, 488, 488}},
      {"LeaveYlo", "free", {488, 488, 488, 488, -152, 488}},
      {"LeaveYhi", "free", {488, 488, 488, 488, 1128, 488}},
      {"LeaveZlo", "free", {488, 488, 488, 488, 488, -152}},
      {"LeaveZhi", "free", {488, 488, 488, 488, 488, 1128}},
      {"StartOutside", "free", {-152, 488, 488, 488, 488, 488}},
      {"StartOutsideHit", "d", {-152, 88, 88, 488, 88, 88}},
      {"WhollyOutside", "free", {-168, -168, -168, -24, -40, -8}},
      {"ZeroLengthInside", "a", {168, 168, 168, 168, 168, 168}},
      {"ZeroLengthFree", "free", {168, 168, 168, 168, 168, 168}},
      {"ZeroLengthCorner", "a", {160, 160, 160, 160, 160, 160}},
      {"LimitLow", "d", {-L, 88, 88, L, 88, 88}},
      {"LimitHigh", "d", {L, 88, 88, -L, 88, 88}},
      {"BeyondLimit", "d", {L + 1, 88, 88, 0, 88, 88}},
  };
  for (const Case& c : cases) {
    const Map& m = *maps[c.map];
    bool is_short = true;   // the literal definition enumerates the bounding box
    for (int k = 0; k < 6; ++k) is_short = is_short && std::abs(c.seg[k]) < 4096;
    trace_result r[2];
    for (int s = 0; s < 2; ++s)
      if (!agree(m, c.seg, kTest, s ? collision_status::unseen : collision_status::occupied, is_short, &r[s])) {
        std::fprintf(stderr, "%s: the walks and the literal definition differ (stop_at %d)\n", c.name.c_str(), s);
        return 1;
      }
    std::printf("%s %d", c.name.c_str(), r[0].valid ? 1 : 0);
    for (int s = 0; s < 2; ++s)
      std::printf(" %d %lld %lld %d %d %d %d %d", r[s].valid ? (int)r[s].status : 255, (long long)r[s].t_first.num, (long long)r[s].t_first.den, r[s].first[0],
                  r[s].first[1], r[s].first[2], r[s].unseen, r[s].empty);
    std::printf("\n");
  }
  return 0;
}

template <typename T>
static void random_map(std::mt19937& rng, int t, long* checked, long* bad) {
  typedef typename voxel_traits<T>::value_type V;
  const se::geometry::voxel_test<T> test = {5.f, false};
  const int size = 64, S = 16 * size;
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
  auto span = [&](int m_) { return (int)(rng() % (unsigned)(2 * m_ + 1)) - m_; };
  for (int k = 0; k < 300; ++k) {
    int32_t seg[6];
    const int kind = k % 6;   // 0: arbitrary, 1: corners along a diagonal, 2: corners, 3: half-voxels, 4: axis-parallel, 5: a point
    const int axis = (int)(rng() % 3);
    const int len = 16 * (1 + (int)(rng() % 12));
    for (int a = 0; a < 3; ++a) {
      seg[a] = (int)(rng() % (unsigned)(S + 640)) - 320;
      seg[3 + a] = seg[a] + span(200);
      if (kind == 1 || kind == 2) seg[a] = seg[a] / 16 * 16;
      if (kind == 1) seg[3 + a] = seg[a] + ((rng() & 1) ? len : -len);
      if (kind == 2) seg[3 + a] = seg[a] + 16 * span(10);
      if (kind == 3) { seg[a] = seg[a] / 16 * 16 + 8; seg[3 + a] = seg[a] + 16 * span(10); }
      if (kind == 4 && a != axis) seg[3 + a] = seg[a];
      if (kind == 5) seg[3 + a] = seg[a];
    }
    if (kind == 1 && k % 12 == 1) { seg[axis] += 5; seg[3 + axis] = seg[axis]; }   // a face diagonal in a slice that is no grid plane
    const collision_status stop = (k / 6) % 2 ? collision_status::unseen : collision_status::occupied;
    ++*checked;
    if (!agree(*m, seg, test, stop, true, nullptr)) {
      if (*bad < 5) std::fprintf(stderr, "map %d segment (%d %d %d | %d %d %d) stop_at %d: the walks and the literal definition differ\n", t, seg[0], seg[1], seg[2],
                                 seg[3], seg[4], seg[5], (int)stop);
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
