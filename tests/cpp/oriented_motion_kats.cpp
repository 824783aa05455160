/*
 * Known-answer and randomised tests of the oriented motion collision queries on the host mirror (include/se/oriented_motion.hpp): the
 * predicate's two forms against each other, and the recursive traversal against the literal definition (every voxel of the bounding box of
 * the sweep).
 *
 *   oriented_motion_kats kats               the hand-worked cases of tests/oriented_motion_util.py on 64^3 SDF maps; one line per case:
 *                                           "<name> <valid> <status> <num> <den> <status> <num> <den>" -- with stop_at occupied, then unseen
 *                                           (status 0 occupied, 1 unseen, 2 empty, 255 invalid; t_exact in lowest terms).  A case whose
 *                                           traversal and brute force differ, or one of whose voxels the interval form and the 21-axis form
 *                                           judge differently, ends the program with 1 (the Limit* cases, which sweep 16 384 voxels, run
 *                                           the traversal only).
 *   oriented_motion_kats random <n> <seed>  n random 64^3 maps (both fields in turn) x 150 motions x both stop_at; prints
 *                                           "checked <k> mismatches <m> forms <cubes> differ <m> occupied <n> unseen <n> empty <n> invalid <n> blocked <n>"
 *
 * Values: x = 10 empty, x = 2 occupied, initValue() unseen, judged by voxel_test{5, below} (as tests/cpp/oriented_kats.cpp).
 *
 * The hand cases.  Voxel (10, 10, 10) is the cube [160, 176)^3 of sub-units.  D is the diamond h0 = (32, 32, 0), h1 = (-32, 32, 0),
 * h2 = (0, 0, 4): the points with |x - c_x| + |y - c_y| < 64, |z - c_z| < 4.
 *   AlignedIntoVoxel   the box [120, 136) x [160, 176)^2 moves 64 along x: its face 136 + 64 t passes 160 at t = 24 / 64 = 3 / 8.
 *   VertexSlidesOn     about (96, 160) the right vertex (160, 160) is the voxel's corner; it moves along x by 16 t, and the point
 *                      (160 + e, 160 + e) lies in the diamond as soon as 2 e < 16 t: touched for every t > 0, t_in = 0 -- an infimum, the
 *                      static query at t = 0 says empty (DiamondVertexOnCorner of oriented_kats.cpp).
 *   VertexSlidesOff    the same diamond moves down: it keeps |x - 96| < 64, so it stays in x < 160 and never touches the voxel.
 *   VertexArrives      about (32, 160), moving 128 along x: the right vertex 96 + 128 t reaches the corner (160, 160) at t = 1 / 2 and slides
 *                      on from there.
 *   FlankArrives       about (32, 152): the flank (x - c_x) + (y - c_y) = 64 meets the corner (160, 160) when (128 - 128 t) + 8 = 64:
 *                      t = 72 / 128 = 9 / 16.
 *   FlankGrazes        about (32, 96): the top vertex runs along y = 160, the diamond stays in y < 160: the voxel is never touched.
 *   StopsShort / At / Past   FlankArrives with d = (71 / 72 / 73, 0, 0): the flank meets the corner at t = 72 / d_x -- beyond 1; at 1, which the
 *                      open condition L < 1 excludes; at 72 / 73.
 *   (Those six diamonds about x = 32 span x in (-32, 96): a part of them is outside the volume from the start.  Where the voxel is not
 *   touched their status is therefore unseen, not empty, and with stop_at unseen they are blocked at t = 0.)
 *   DiagonalApproach   about (40, 40), moving (200, 200): the flank meets the corner when (120 - 200 t) + (120 - 200 t) = 64: t = 11 / 25.
 *   SkewMoves          the parallelogram c + s0 (16, 0) + s1 (16, 16) about (230, 160), moving -60 along x: for y = 160 + 16 s1 in the voxel's
 *                      range its left edge is c_x + 16 s1 - 16 > c_x - 16, so the voxel (x < 176) is touched iff c_x < 192: 230 - 60 t < 192,
 *                      t > 38 / 60 = 19 / 30 (SkewMisses of oriented_kats.cpp is the same box at c_x = 192).
 *   Rot345             R10 = (40, 30, 0), (-30, 40, 0), (0, 0, 50) about (100, 120, 150), moving (100, 90, 40).  Along the face normal
 *                      u = (4, 3, 0) / 5 the box has half width 50, the voxel 8 (4 + 3) / 5 = 11.2, their centres are (4 * 68 + 3 * 48) / 5 =
 *                      83.2 apart and close at u . d = 134: 83.2 - 134 t = 61.2 gives t = 22 / 134 = 11 / 67; every other axis overlaps by then.
 *   Rot345Back         about (300, 290, 200), moving (-200, -170, -50): the centres are 178.8 apart along u and close at 262:
 *                      178.8 - 262 t = 61.2 gives t = 117.6 / 262 = 294 / 655.
 *   Leave*             R = (4, 3, 0), (-3, 4, 0), (0, 0, 5) about (168, 168, 168) has ext = (7, 7, 5).  Moving 400 towards a low face it
 *                      reaches 0 at (168 - ext_k) / 400; moving 900 towards a high face it reaches 1024 at (1024 - 168 - ext_k) / 900 =
 *                      849 / 900 (x, y) or 851 / 900 (z).  With stop_at occupied nothing blocks.  StaysInside: the same box, inside all along.
 *   OctantEnters       on the octant map R10 about (160, 640, 640) starts in the unseen absent octants of the root and moves 400 along x: its
 *                      vertex c + h0 - h1 = c + (70, -10, 0) reaches the occupied node [512, 768)^3 at (512 - 230) / 400 = 141 / 200.
 *                      OctantStopsBefore: d_x = 282 ends exactly there (t = 1: not touched).  OctantInside: wholly inside the node.
 *   IntoWall           the wall is x in [320, 336); the diamond about (100, 500) moves (200, 30, 7), its right vertex 164 + 200 t reaches 320
 *                      at 156 / 200 = 39 / 50.  AlongWall: about x = 256 the right vertex is at 320 and slides along the wall's face.
 *   LimitMoveUp / Down a voxel-sized box crosses the whole valid displacement onto the voxel: from 200 - 2^18 its face c_x + 8 reaches 160 at
 *                      (2^18 - 48) / 2^18 = 16381 / 16384; from 100 + 2^18 its face c_x - 8 reaches 176 at (2^18 - 84) / 2^18 = 65515 / 65536.
 *   LimitCentreEnd     c_x + d_x = 2^20 exactly: valid, far outside.   Invalid*: |d_k| = 2^18 + 1, |c_k + d_k| = 2^20 + 1, det = 0,
 *                      |c_k| = 2^20 + 1, |h_ik| = 2^14 + 1, INT32_MIN components.
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
#include "se/oriented_motion.hpp"

using se::geometry::collision_status;
using se::geometry::int3;
using se::geometry::oriented_motion;
using se::geometry::oriented_motion_result;
using se::geometry::rational;

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

/* a 64^3 map with every block allocated and every voxel empty, then the listed voxels and the plane x = wall (if >= 0) occupied */
static std::unique_ptr<Map> free_map(const std::vector<int3>& occupied, int wall = -1) {
  Builder<SDF> b(64);
  for (int z = 0; z < 64; z += 8)
    for (int y = 0; y < 64; y += 8)
      for (int x = 0; x < 64; x += 8) b.allocate(x, y, z);
  auto m = b.build();
  for (auto& bl : m->getBlockBuffer())
    for (int v = 0; v < 512; ++v) bl->voxel_block_[v].x = 10.f;
  std::vector<int3> occ = occupied;
  if (wall >= 0)
    for (int z = 0; z < 64; ++z)
      for (int y = 0; y < 64; ++y) occ.push_back({{wall, y, z}});
  for (const int3& o : occ) {
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

struct Case { const char* name; const char* map; int32_t m[15]; };

static bool same_result(const oriented_motion_result& a, const oriented_motion_result& d) {
  if (a.valid != d.valid) return false;
  return !a.valid || (a.status == d.status && a.t_exact.num == d.t_exact.num && a.t_exact.den == d.t_exact.den);
}

/* traversal == brute force, for one stop_at */
template <typename T, typename TestF>
static bool same(const se::Octree<T>& m, const oriented_motion& mo, TestF test, collision_status stop, oriented_motion_result* out) {
  const oriented_motion_result a = se::geometry::oriented_motion_status(m, mo, test, stop);
  const oriented_motion_result d = se::geometry::oriented_motion_status_brute(m, mo, test, stop);
  if (out) *out = a;
  return same_result(a, d);
}

/* the interval form against the 21-axis form on every voxel about the sweep and on every larger cube, up to side `size`, that meets that
 * region: the cubes compared, -1 if they differ */
static long forms_agree(const oriented_motion& mo, int size) {
  if (!se::geometry::oriented_motion_valid(mo)) return 0;
  long cubes = 0;
  int lo[3], hi[3];
  for (int k = 0; k < 3; ++k) {
    const int64_t ext = se::geometry::oriented_detail::extent(mo.box, k);
    const int64_t a = mo.box.c[k] - ext + (mo.d[k] < 0 ? mo.d[k] : 0), b = mo.box.c[k] + ext + (mo.d[k] > 0 ? mo.d[k] : 0);
    lo[k] = (int)std::floor((double)a / 16) - 2;
    hi[k] = (int)std::ceil((double)b / 16) + 2;
  }
  for (int s = 1; s <= size; s *= 2) {   // the cubes of side s on the grid of that side that meet the region
    int g0[3];
    for (int k = 0; k < 3; ++k) g0[k] = (int)std::floor((double)lo[k] / s) * s;
    for (int z = g0[2]; z < hi[2]; z += s)
      for (int y = g0[1]; y < hi[1]; y += s)
        for (int x = g0[0]; x < hi[0]; x += s) {
          const int v[3] = {x, y, z};
          ++cubes;
          if (se::geometry::oriented_motion_entry(mo.box, mo.d, v, s, nullptr) != se::geometry::oriented_motion_swept(mo.box, mo.d, v, s)) return -1;
        }
  }
  return cubes;
}

static int run_kats() {
  std::map<std::string, std::unique_ptr<Map>> maps;
  maps["a"] = free_map({{{10, 10, 10}}});
  maps["free"] = free_map({});
  maps["wall"] = free_map({}, 20);
  maps["octant"] = octant_map();
  const int CL = se::geometry::oriented_centre_limit, HL = se::geometry::oriented_axis_limit, ML = se::geometry::oriented_move_limit;
  const int32_t MIN = INT32_MIN;
#define A8 8, 0, 0, 0, 8, 0, 0, 0, 8
#define DD 32, 32, 0, -32, 32, 0, 0, 0, 4
#define RR 4, 3, 0, -3, 4, 0, 0, 0, 5
#define R10 40, 30, 0, -30, 40, 0, 0, 0, 50
  const Case cases[] = {
      {"AlignedIntoVoxel", "a", {128, 168, 168, A8, 64, 0, 0}},
      {"VertexSlidesOn", "a", {96, 160, 168, DD, 16, 0, 0}},
      {"VertexSlidesOff", "a", {96, 160, 168, DD, 0, -16, 0}},
      {"VertexArrives", "a", {32, 160, 168, DD, 128, 0, 0}},
      {"FlankArrives", "a", {32, 152, 168, DD, 128, 0, 0}},
      {"FlankGrazes", "a", {32, 96, 168, DD, 128, 0, 0}},
      {"StopsShort", "a", {32, 152, 168, DD, 71, 0, 0}},
      {"StopsAt", "a", {32, 152, 168, DD, 72, 0, 0}},
      {"StopsPast", "a", {32, 152, 168, DD, 73, 0, 0}},
      {"DiagonalApproach", "a", {40, 40, 168, DD, 200, 200, 0}},
      {"SkewMoves", "a", {230, 160, 168, 16, 0, 0, 16, 16, 0, 0, 0, 8, -60, 0, 0}},
      {"Rot345", "a", {100, 120, 150, R10, 100, 90, 40}},
      {"Rot345Back", "a", {300, 290, 200, R10, -200, -170, -50}},
      {"LeaveXlo", "free", {168, 168, 168, RR, -400, 0, 0}},
      {"LeaveYlo", "free", {168, 168, 168, RR, 0, -400, 0}},
      {"LeaveZlo", "free", {168, 168, 168, RR, 0, 0, -400}},
      {"LeaveXhi", "free", {168, 168, 168, RR, 900, 0, 0}},
      {"LeaveYhi", "free", {168, 168, 168, RR, 3, 900, 0}},
      {"LeaveZhi", "free", {168, 168, 168, RR, 0, -5, 900}},
      {"StaysInside", "free", {168, 168, 168, RR, 100, 50, -20}},
      {"OctantEnters", "octant", {160, 640, 640, R10, 400, 0, 0}},
      {"OctantStopsBefore", "octant", {160, 640, 640, R10, 282, 0, 0}},
      {"OctantInside", "octant", {640, 640, 640, R10, 10, 10, 10}},
      {"IntoWall", "wall", {100, 500, 500, DD, 200, 30, 7}},
      {"AlongWall", "wall", {256, 500, 500, DD, 0, 300, 100}},
      {"LimitMoveUp", "a", {200 - ML, 168, 168, A8, ML, 0, 0}},
      {"LimitMoveDown", "a", {100 + ML, 168, 168, A8, -ML, 0, 0}},
      {"LimitCentreEnd", "a", {CL - 11, 168, 168, RR, 11, 0, 0}},
      {"InvalidMove", "a", {168, 168, 168, RR, ML + 1, 0, 0}},
      {"InvalidMoveLow", "a", {168, 168, 168, RR, 0, 0, -ML - 1}},
      {"InvalidEnd", "a", {CL - 10, 168, 168, RR, 11, 0, 0}},
      {"InvalidEndLow", "a", {168, -CL + 10, 168, RR, 0, -11, 0}},
      {"InvalidDet", "a", {168, 168, 168, 8, 8, 0, 1, 0, 0, 8, 8, 0, 16, 0, 0}},
      {"InvalidCentre", "a", {CL + 1, 168, 168, RR, -16, 0, 0}},
      {"InvalidAxis", "a", {168, 168, 168, HL + 1, 0, 0, 0, 8, 0, 0, 0, 8, 16, 0, 0}},
      {"InvalidInt32MinMove", "a", {168, 168, 168, RR, MIN, MIN, MIN}},
      {"InvalidInt32MinCentre", "a", {MIN, 168, 168, RR, MIN, 0, 0}},
      {"InvalidInt32MinAxes", "a", {168, 168, 168, MIN, MIN, MIN, 0, MIN, 0, 0, 0, MIN, 0, 0, 0}},
  };
  for (const Case& c : cases) {
    const Map& m = *maps[c.map];
    const oriented_motion mo = se::geometry::oriented_motion_from(c.m);
    const bool limit = std::string(c.name).compare(0, 5, "Limit") == 0;
    oriented_motion_result r[2];
    for (int s = 0; s < 2; ++s) {
      const collision_status stop = s == 0 ? collision_status::occupied : collision_status::unseen;
      if (limit) {
        r[s] = se::geometry::oriented_motion_status(m, mo, kTest, stop);
      } else if (!same(m, mo, kTest, stop, &r[s])) {
        std::fprintf(stderr, "%s: traversal and brute force differ\n", c.name);
        return 1;
      }
    }
    if (!limit && forms_agree(mo, 64) < 0) {
      std::fprintf(stderr, "%s: the interval form and the 21-axis form differ\n", c.name);
      return 1;
    }
    std::printf("%s %d", c.name, r[0].valid ? 1 : 0);
    for (int s = 0; s < 2; ++s) std::printf(" %d %lld %lld", r[s].valid ? (int)r[s].status : 255, (long long)r[s].t_exact.num, (long long)r[s].t_exact.den);
    std::printf("\n");
  }
  return 0;
}

struct Tally { long checked = 0, bad = 0, cubes = 0, differ = 0, seen[4] = {0, 0, 0, 0}, blocked = 0; };

template <typename T>
static void random_map(std::mt19937& rng, int t, Tally& y) {
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
  for (int k = 0; k < 150; ++k) {
    oriented_motion mo;
    se::geometry::oriented_box& bx = mo.box;
    const int kind = k % 8;   // 0: axis-aligned on voxel boundaries moved by whole voxels, 1: axis-aligned anywhere, 2: skew, else rotated
    for (int a = 0; a < 3; ++a) bx.c[a] = (int)(rng() % (unsigned)((size + 16) * sub)) - 8 * sub;
    double len[3];
    for (int a = 0; a < 3; ++a) len[a] = std::exp(uni(rng) * std::log(4.0 * sub));   // 1 / 16 voxel .. 4 voxels
    if (kind <= 1) {
      for (int i = 0; i < 3; ++i)
        for (int a = 0; a < 3; ++a) bx.h[i][a] = i == a ? (kind == 0 ? (sub / 2) * (1 + (int)(rng() % 6)) : 1 + (int)len[i]) : 0;
      if (kind == 0)
        for (int a = 0; a < 3; ++a) bx.c[a] = (bx.c[a] / sub) * sub + (bx.h[a][a] % sub);
    } else {
      double q[4], nrm = 0;
      for (int a = 0; a < 4; ++a) { q[a] = normal(rng); nrm += q[a] * q[a]; }
      nrm = std::sqrt(nrm);
      const double w = q[0] / nrm, x = q[1] / nrm, yy = q[2] / nrm, z = q[3] / nrm;
      const double R[3][3] = {{1 - 2 * (yy * yy + z * z), 2 * (x * yy - z * w), 2 * (x * z + yy * w)},
                              {2 * (x * yy + z * w), 1 - 2 * (x * x + z * z), 2 * (yy * z - x * w)},
                              {2 * (x * z - yy * w), 2 * (yy * z + x * w), 1 - 2 * (x * x + yy * yy)}};
      for (int i = 0; i < 3; ++i)
        for (int a = 0; a < 3; ++a) bx.h[i][a] = (int)std::nearbyint(R[a][i] * len[i] + (kind == 2 && i == 1 ? 0.5 * R[a][0] * len[0] : 0.0));
    }
    // the displacement: up to 12 voxels; every fifth with a zero component, every seventh none at all, every eleventh along a half-axis
    for (int a = 0; a < 3; ++a) mo.d[a] = kind == 0 ? sub * ((int)(rng() % 17) - 8) : (int)(rng() % (unsigned)(24 * sub + 1)) - 12 * sub;
    if (k % 5 == 0) mo.d[rng() % 3] = 0;
    if (k % 7 == 0) mo.d[0] = mo.d[1] = mo.d[2] = 0;
    if (k % 11 == 0) { const int i = (int)(rng() % 3), f = (int)(rng() % 5) - 2; for (int a = 0; a < 3; ++a) mo.d[a] = f * bx.h[i][a]; }
    ++y.checked;   // (a box whose rounded axes are dependent is invalid: both sides must say so)
    oriented_motion_result r[2];
    bool ok = true;
    for (int s = 0; s < 2; ++s) ok = same(*m, mo, test, s == 0 ? collision_status::occupied : collision_status::unseen, &r[s]) && ok;
    ok = ok && r[0].status == r[1].status;
    const long cubes = forms_agree(mo, size);
    if (cubes < 0) ++y.differ; else y.cubes += cubes;
    ++y.seen[r[0].valid ? (int)r[0].status : 3];
    if (r[0].valid && r[0].t_exact.num > 0 && r[0].t_exact.num < r[0].t_exact.den) ++y.blocked;
    if (!ok || cubes < 0) {
      if (y.bad < 5) {
        std::fprintf(stderr, "map %d motion (", t);
        for (int a = 0; a < 3; ++a) std::fprintf(stderr, "%d ", bx.c[a]);
        for (int i = 0; i < 3; ++i)
          for (int a = 0; a < 3; ++a) std::fprintf(stderr, "%d ", bx.h[i][a]);
        for (int a = 0; a < 3; ++a) std::fprintf(stderr, "%d ", mo.d[a]);
        std::fprintf(stderr, "): %s\n", cubes < 0 ? "the two forms differ" : "traversal and brute force differ");
      }
      ++y.bad;
    }
  }
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "kats";
  if (mode == "kats") return run_kats();
  if (mode == "random") {
    const int n = argc > 2 ? std::atoi(argv[2]) : 4;
    std::mt19937 rng(argc > 3 ? (unsigned)std::atoi(argv[3]) : 1u);
    Tally y;
    for (int t = 0; t < n; ++t) {
      if (t % 2) random_map<OFusion>(rng, t, y);
      else random_map<SDF>(rng, t, y);
    }
    std::printf("checked %ld mismatches %ld forms %ld differ %ld occupied %ld unseen %ld empty %ld invalid %ld blocked %ld\n", y.checked, y.bad, y.cubes, y.differ,
                y.seen[0], y.seen[1], y.seen[2], y.seen[3], y.blocked);
    return y.bad ? 1 : 0;
  }
  return 2;
}
