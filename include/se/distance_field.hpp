/*
 * The distance field of a map region on the host se::Octree snapshot that DenseSLAMSystem::getMap() materialises: the executable
 * definition of se_hip_distance_field (include/se_hip.h), without Eigen, beside clearance.hpp.
 *
 * For every voxel v of the region [lo, lo + side) the field holds the clearance (clearance.hpp) of the box [v, v + robot) with r_max:
 * the smallest d2 = g_x^2 + g_y^2 + g_z^2 <= r_max^2 over the blocking voxels c, g_k = max(0, c_k - (v_k + robot_k), v_k - (c_k + 1)), and
 * among the voxels that attain it the smallest in (z, y, x) order.
 *
 * Two things are provided:
 *   distance_field_brute(map, request, test, stop_at)  (a) the definition, literally: per voxel of the region every candidate of the box
 *                                                      dilated by r_max + 1, each with the gap formula and Octree::get, folded
 *                                                      lexicographically (clearance_detail::fold).
 *   distance_field(map, request, test, stop_at)        (b) the three-pass restatement that the device follows.  The gap is per axis, so d2
 *                                                      is a min-plus product: an x pass keeps per row (c_y, c_z) the candidate that
 *                                                      minimises (g_x^2, c_x); a y pass keeps per (c_z) the minimum of (g_x^2 + g_y^2, c_y,
 *                                                      c_x) over those; a z pass the minimum of (d2, c_z, c_y, c_x).  A candidate that is
 *                                                      not minimal in its own line cannot attain the minimum of the sum, so nothing is
 *                                                      lost.  With o = c - v a gap is at most r_max exactly for o in [-1 - r_max, robot +
 *                                                      r_max]: per axis only the domain [lo - 1 - r_max, lo + side - 1 + robot + r_max]
 *                                                      (D = side + robot + 2 r_max + 1 cells) is classified, once.  The last pass applies
 *                                                      d2 <= r_max^2.
 * Both return d2 [side z][side y][side x] and nearest [..][3] (x y z) in the layout of the device's outputs; an invalid request
 * (field_valid: the refusals of se_hip_distance_field) returns false and leaves them empty.
 */
#ifndef SE_HIP_DISTANCE_FIELD_HPP
#define SE_HIP_DISTANCE_FIELD_HPP

#include <climits>
#include <cstdint>
#include <vector>

#include "clearance.hpp"
#include "octree.hpp"
#include "octree_collision.hpp"

namespace se {
namespace geometry {

constexpr int field_r_max = 255;               /* largest r_max of a valid request */
constexpr int field_robot_max = 256;           /* largest robot side */
constexpr int64_t field_max_voxels = 1 << 24;  /* side_x side_y side_z */
constexpr int64_t field_max_work = 1 << 28;    /* side_x D_y D_z */

struct field_request {
  int3 lo, side, robot;
  int r_max;
};

struct field_result {
  std::vector<int32_t> d2;       /* [side z][side y][side x]; clearance_none */
  std::vector<int32_t> nearest;  /* [side z][side y][side x][3]; INT32_MIN three times for none */
};

inline bool region_valid(const int3& lo, const int3& side, const int3& robot) {   /* what every request over a region must satisfy */
  int64_t voxels = 1;
  for (int k = 0; k < 3; ++k) {
    const int64_t a = lo(k), b = (int64_t)lo(k) + side(k) + robot(k);
    if (side(k) < 1 || robot(k) < 1 || robot(k) > field_robot_max || a < -clearance_limit || b > clearance_limit) return false;   /* (a < b by then) */
    voxels *= side(k);
  }
  return voxels <= field_max_voxels;
}
inline bool field_valid(const field_request& q) {
  const int64_t w = 2 * (int64_t)q.r_max + 1, d1 = w + q.side(1) + q.robot(1), d2 = w + q.side(2) + q.robot(2);
  return q.r_max >= 0 && q.r_max <= field_r_max && region_valid(q.lo, q.side, q.robot) && q.side(0) * d1 * d2 <= field_max_work;
}

namespace field_detail {
template <typename T, typename TestF>
inline bool blocks(const Octree<T>& map, const int x, const int y, const int z, TestF test, const collision_status stop_at) {
  const int n = map.size();
  const bool in = x >= 0 && y >= 0 && z >= 0 && x < n && y < n && z < n;
  return (int)(in ? test(map.get(x, y, z)) : collision_status::unseen) <= (int)stop_at;
}
/* the gap of a candidate at offset o = c - v from a box of side `robot` at v */
inline int gap_of(const int o, const int robot) { return o > robot ? o - robot : (o < -1 ? -o - 1 : 0); }
constexpr int none = INT_MIN;   /* "no candidate" in the pass buffers */
}  // namespace field_detail

/* (a) the definition */
template <typename T, typename TestF>
bool distance_field_brute(const Octree<T>& map, const field_request& q, TestF test, const collision_status stop_at, field_result& out) {
  out.d2.clear(); out.nearest.clear();
  if (!field_valid(q)) return false;
  const int m = q.r_max + 1;
  for (int k = 0; k < q.side(2); ++k)
    for (int j = 0; j < q.side(1); ++j)
      for (int i = 0; i < q.side(0); ++i) {
        const int3 v = {{q.lo(0) + i, q.lo(1) + j, q.lo(2) + k}};
        clearance_detail::fold f;
        f.limit = (int64_t)q.r_max * q.r_max;
        for (int z = v(2) - m; z < v(2) + q.robot(2) + m; ++z)
          for (int y = v(1) - m; y < v(1) + q.robot(1) + m; ++y)
            for (int x = v(0) - m; x < v(0) + q.robot(0) + m; ++x) {
              const int3 c = {{x, y, z}};
              if (field_detail::blocks(map, x, y, z, test, stop_at)) f.add(cube_d2(v, q.robot, c, 1), c);
            }
        const clearance_result r = f.result();
        out.d2.push_back((int32_t)r.d2);
        for (int a = 0; a < 3; ++a) out.nearest.push_back(r.nearest(a));
      }
  return true;
}

/* (b) the three passes */
template <typename T, typename TestF>
bool distance_field(const Octree<T>& map, const field_request& q, TestF test, const collision_status stop_at, field_result& out) {
  using field_detail::gap_of;
  using field_detail::none;
  out.d2.clear(); out.nearest.clear();
  if (!field_valid(q)) return false;
  const int r = q.r_max;
  const size_t s0 = (size_t)q.side(0), s1 = (size_t)q.side(1), s2 = (size_t)q.side(2);
  size_t D[3];
  int o[3];   /* the domain's first voxel */
  for (int k = 0; k < 3; ++k) { D[k] = (size_t)(q.side(k) + q.robot(k) + 2 * r + 1); o[k] = q.lo(k) - 1 - r; }
  /* the domain, classified once */
  std::vector<uint8_t> blk(D[0] * D[1] * D[2]);
  for (size_t z = 0; z < D[2]; ++z)
    for (size_t y = 0; y < D[1]; ++y)
      for (size_t x = 0; x < D[0]; ++x)
        blk[(z * D[1] + y) * D[0] + x] = field_detail::blocks(map, o[0] + (int)x, o[1] + (int)y, o[2] + (int)z, test, stop_at) ? 1 : 0;
  /* x: per (i, y, z) the offset c_x - v_x that minimises (g_x^2, c_x): the lowest candidate of the zero-gap interval [-1, robot], else the
   * nearer of the nearest below and the nearest above within r_max, the lower one at equal gaps */
  std::vector<int> ax(s0 * D[1] * D[2], none);
  for (size_t z = 0; z < D[2]; ++z)
    for (size_t y = 0; y < D[1]; ++y) {
      const uint8_t* row = &blk[(z * D[1] + y) * D[0]];
      for (size_t i = 0; i < s0; ++i) {
        const int pv = 1 + r + (int)i;   /* v_x in the row */
        int best = none;
        for (int c = pv - 1; c <= pv + q.robot(0) && best == none; ++c)
          if (row[c]) best = c - pv;
        if (best == none) {
          int below = none, above = none;
          for (int c = pv - 2; c >= pv - 1 - r && below == none; --c)
            if (row[c]) below = c - pv;
          for (int c = pv + q.robot(0) + 1; c <= pv + q.robot(0) + r && above == none; ++c)
            if (row[c]) above = c - pv;
          if (below != none && (above == none || gap_of(below, q.robot(0)) <= gap_of(above, q.robot(0)))) best = below;
          else best = above;
        }
        ax[(z * D[1] + y) * s0 + i] = best;
      }
    }
  /* y: per (i, j, z) the pair of offsets that minimises (g_x^2 + g_y^2, c_y, c_x): candidates ascending, the first strict minimum */
  std::vector<int> ay_x(s0 * s1 * D[2], none), ay_y(s0 * s1 * D[2], none);
  for (size_t z = 0; z < D[2]; ++z)
    for (size_t j = 0; j < s1; ++j)
      for (size_t i = 0; i < s0; ++i) {
        int64_t best = INT64_MAX;
        for (int t = 0; t < q.robot(1) + 2 * r + 2; ++t) {
          const int ox = ax[(z * D[1] + j + (size_t)t) * s0 + i];
          if (ox == none) continue;
          const int oy = t - 1 - r;
          const int64_t gx = gap_of(ox, q.robot(0)), gy = gap_of(oy, q.robot(1)), cost = gx * gx + gy * gy;
          if (cost < best) { best = cost; ay_x[(z * s1 + j) * s0 + i] = ox; ay_y[(z * s1 + j) * s0 + i] = oy; }
        }
      }
  /* z: the same over c_z, then d2 <= r_max^2 */
  out.d2.resize(s0 * s1 * s2);
  out.nearest.resize(3 * s0 * s1 * s2);
  for (size_t k = 0; k < s2; ++k)
    for (size_t j = 0; j < s1; ++j)
      for (size_t i = 0; i < s0; ++i) {
        int64_t best = INT64_MAX;
        int b[3] = {0, 0, 0};
        for (int t = 0; t < q.robot(2) + 2 * r + 2; ++t) {
          const size_t at = ((k + (size_t)t) * s1 + j) * s0 + i;
          if (ay_x[at] == none) continue;
          const int oz = t - 1 - r;
          const int64_t gx = gap_of(ay_x[at], q.robot(0)), gy = gap_of(ay_y[at], q.robot(1)), gz = gap_of(oz, q.robot(2)), cost = gx * gx + gy * gy + gz * gz;
          if (cost < best) { best = cost; b[0] = ay_x[at]; b[1] = ay_y[at]; b[2] = oz; }
        }
        const size_t at = (k * s1 + j) * s0 + i;
        const bool found = best <= (int64_t)r * r;
        const int v[3] = {q.lo(0) + (int)i, q.lo(1) + (int)j, q.lo(2) + (int)k};
        out.d2[at] = found ? (int32_t)best : (int32_t)clearance_none;
        for (int a = 0; a < 3; ++a) out.nearest[3 * at + a] = found ? v[a] + b[a] : INT32_MIN;
      }
  return true;
}

}  // namespace geometry
}  // namespace se

#endif /* SE_HIP_DISTANCE_FIELD_HPP */
