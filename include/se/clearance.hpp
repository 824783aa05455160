/*
 * Clearance queries -- the nearest blocking voxel to a box -- on the host se::Octree snapshot that DenseSLAMSystem::getMap() materialises:
 * the executable definition of se_hip_clearance_boxes (include/se_hip.h), without Eigen, beside motion_collision.hpp.
 *
 * The box is [lo, lo + side) in whole voxels.  For a cube with integer corner c and side s (a voxel: s = 1) the gap on axis k is
 *     g_k = max(0, c_k - (lo_k + side_k), lo_k - (c_k + s))
 * and d2 = g_x^2 + g_y^2 + g_z^2 is the squared Euclidean distance between the two closed sets (0 when they overlap or touch).  The voxels
 * of a cube that attain the cube's d2 are a product of per-axis intervals; the smallest of them in (z, y, x) order has per axis the lowest
 * coordinate of that interval: c if the cube lies above the box, c + s - 1 if it lies below, max(lo - 1, c) otherwise (cube_low).  So every
 * voxel of a cube has a pair (d2, (z, y, x)) that is not smaller, lexicographically, than (the cube's d2, the cube's lowest nearest voxel):
 * a traversal may skip a cube whose pair is not smaller than the best found so far.
 *
 * Three things are provided:
 *   gap / cube_d2 / cube_low / cube_witness         the formulas;
 *   clearance(map, lo, side, r_max, test, stop_at)  a plain recursive pruned traversal of the octree, the volume's outside in closed form;
 *   clearance_brute(map, ...)                       the definition, literally: every voxel of the box dilated by r_max + 1.  This is the
 *                                                   model the traversal and the device are held to.
 * Classification is that of se_hip_collide_boxes in strict mode: test(Octree::get(v)) inside [0, size)^3, unseen outside.  A voxel blocks
 * when its class is <= stop_at (occupied, or unseen: unseen and occupied).  The answer is the smallest d2 <= r_max^2 over the blocking
 * voxels and, among those that attain it, the smallest in (z, y, x) order.
 */
#ifndef SE_HIP_CLEARANCE_HPP
#define SE_HIP_CLEARANCE_HPP

#include <cstdint>

#include "octree.hpp"
#include "octree_collision.hpp"

namespace se {
namespace geometry {

constexpr int clearance_limit = 1 << 19;   /* |coordinate| bound of lo and lo + side of a valid query */
constexpr int clearance_r_max = 32767;     /* largest r_max of a valid query */
constexpr int64_t clearance_none = -1;     /* d2 when nothing blocks within r_max: SE_HIP_CLEARANCE_NONE */
constexpr int64_t clearance_invalid = -2;  /* d2 of an invalid query: SE_HIP_CLEARANCE_INVALID */

struct clearance_result {
  int64_t d2;     /* clearance_none, clearance_invalid */
  int3 nearest;   /* (INT32_MIN, INT32_MIN, INT32_MIN) for none and for invalid */
};

template <typename Vec3i>
inline bool clearance_valid(const Vec3i& lo, const Vec3i& side, const int r_max) {
  if (r_max < 0 || r_max > clearance_r_max) return false;
  for (int k = 0; k < 3; ++k) {
    const int64_t a = lo(k), b = (int64_t)lo(k) + side(k);
    if (side(k) < 1 || a < -clearance_limit || a > clearance_limit || b < -clearance_limit || b > clearance_limit) return false;
  }
  return true;
}

/* one axis: the gap between the box [lo, lo + side) and the cube [c, c + s) */
inline int64_t gap(const int64_t lo, const int64_t side, const int64_t c, const int64_t s) {
  const int64_t above = c - (lo + side), below = lo - (c + s);
  return above > 0 ? above : (below > 0 ? below : 0);
}
/* one axis: the lowest coordinate among the cube's voxels that attain that gap */
inline int64_t cube_low(const int64_t lo, const int64_t side, const int64_t c, const int64_t s) {
  if (c >= lo + side) return c;
  if (c + s <= lo) return c + s - 1;
  return lo - 1 > c ? lo - 1 : c;
}
template <typename Vec3i, typename Vec3j>
inline int64_t cube_d2(const Vec3i& lo, const Vec3i& side, const Vec3j& c, const int s) {
  int64_t d = 0;
  for (int k = 0; k < 3; ++k) { const int64_t g = gap(lo(k), side(k), c(k), s); d += g * g; }
  return d;
}
template <typename Vec3i, typename Vec3j>
inline int3 cube_witness(const Vec3i& lo, const Vec3i& side, const Vec3j& c, const int s) {
  return {{(int)cube_low(lo(0), side(0), c(0), s), (int)cube_low(lo(1), side(1), c(1), s), (int)cube_low(lo(2), side(2), c(2), s)}};
}

namespace clearance_detail {

/* a before b in (z, y, x) order */
inline bool precedes(const int3& a, const int3& b) {
  for (int k = 2; k >= 0; --k)
    if (a(k) != b(k)) return a(k) < b(k);
  return false;
}

struct fold {
  int64_t limit;       /* r_max^2 */
  bool found = false;
  int64_t d2 = 0;
  int3 nearest = {{0, 0, 0}};
  /* (d, w) could still replace the answer */
  bool better(const int64_t d, const int3& w) const { return d <= limit && (!found || d < d2 || (d == d2 && precedes(w, nearest))); }
  void add(const int64_t d, const int3& w) {
    if (better(d, w)) { found = true; d2 = d; nearest = w; }
  }
  clearance_result result() const {
    if (found) return {d2, nearest};
    return {clearance_none, {{INT32_MIN, INT32_MIN, INT32_MIN}}};
  }
};

/* The voxels outside [0, size)^3, all unseen: six half-spaces.  In v_k <= -1 the nearest voxels have v_k in [lo_k - 1, -1] if that is not
 * empty, else v_k = -1, and on the other axes any coordinate in [lo_j - 1, lo_j + side_j]; in v_k >= size correspondingly. */
template <typename Vec3i>
inline void outside(const int size, const Vec3i& lo, const Vec3i& side, fold& f) {
  for (int k = 0; k < 3; ++k)
    for (int up = 0; up < 2; ++up) {
      const int64_t far = up ? (int64_t)size - (lo(k) + side(k)) : lo(k);
      const int64_t g = far > 0 ? far : 0;
      int3 w = {{lo(0) - 1, lo(1) - 1, lo(2) - 1}};
      if (up) w(k) = lo(k) - 1 > size ? lo(k) - 1 : size;
      else w(k) = lo(k) - 1 < -1 ? lo(k) - 1 : -1;
      f.add(g * g, w);
    }
}

template <typename T, typename Vec3i, typename TestF>
void descend(Node<T>* node, const int x, const int y, const int z, const int s, const Vec3i& lo, const Vec3i& side, TestF test, const collision_status stop_at, fold& f) {
  const int h = s / 2;
  for (int i = 0; i < 8; ++i) {
    const int3 c = {{x + ((i & 1) ? h : 0), y + ((i & 2) ? h : 0), z + ((i & 4) ? h : 0)}};
    const int64_t d = cube_d2(lo, side, c, h);
    const int3 w = cube_witness(lo, side, c, h);
    if (!f.better(d, w)) continue;
    Node<T>* child = node->child(i);
    if (!child) {
      if ((int)test(node->value_[i]) <= (int)stop_at) f.add(d, w);   /* every voxel of the octant reads this value (Octree::get) */
    } else if (child->isLeaf()) {
      const VoxelBlock<T>* b = static_cast<const VoxelBlock<T>*>(child);
      for (int vz = c(2); vz < c(2) + h; ++vz)
        for (int vy = c(1); vy < c(1) + h; ++vy)
          for (int vx = c(0); vx < c(0) + h; ++vx) {
            const int3 v = {{vx, vy, vz}};
            const int64_t dv = cube_d2(lo, side, v, 1);
            if (f.better(dv, v) && (int)test(b->data(vx, vy, vz)) <= (int)stop_at) f.add(dv, v);
          }
    } else {
      descend(child, c(0), c(1), c(2), h, lo, side, test, stop_at, f);
    }
  }
}

}  // namespace clearance_detail

/* The traversal: the nearest blocking voxel within r_max of one box against the whole map. */
template <typename T, typename Vec3i, typename TestF>
clearance_result clearance(const Octree<T>& map, const Vec3i& lo, const Vec3i& side, const int r_max, TestF test, const collision_status stop_at) {
  if (!clearance_valid(lo, side, r_max)) return {clearance_invalid, {{INT32_MIN, INT32_MIN, INT32_MIN}}};
  clearance_detail::fold f;
  f.limit = (int64_t)r_max * r_max;
  if ((int)stop_at >= (int)collision_status::unseen) clearance_detail::outside(map.size(), lo, side, f);
  const int3 origin = {{0, 0, 0}};
  const int64_t d = cube_d2(lo, side, origin, map.size());
  const int3 w = cube_witness(lo, side, origin, map.size());
  if (f.better(d, w)) {
    if (!map.root()) {   /* Octree::get without a root */
      if ((int)test(voxel_traits<T>::initValue()) <= (int)stop_at) f.add(d, w);
    } else {
      clearance_detail::descend(map.root(), 0, 0, 0, map.size(), lo, side, test, stop_at, f);
    }
  }
  return f.result();
}

/* The definition: every voxel of the box dilated by r_max + 1, each with the gap formula and Octree::get. */
template <typename T, typename Vec3i, typename TestF>
clearance_result clearance_brute(const Octree<T>& map, const Vec3i& lo, const Vec3i& side, const int r_max, TestF test, const collision_status stop_at) {
  if (!clearance_valid(lo, side, r_max)) return {clearance_invalid, {{INT32_MIN, INT32_MIN, INT32_MIN}}};
  clearance_detail::fold f;
  f.limit = (int64_t)r_max * r_max;
  const int n = map.size(), m = r_max + 1;
  for (int z = lo(2) - m; z < lo(2) + side(2) + m; ++z)
    for (int y = lo(1) - m; y < lo(1) + side(1) + m; ++y)
      for (int x = lo(0) - m; x < lo(0) + side(0) + m; ++x) {
        const int3 v = {{x, y, z}};
        const bool in = x >= 0 && y >= 0 && z >= 0 && x < n && y < n && z < n;
        const collision_status c = in ? test(map.get(x, y, z)) : collision_status::unseen;
        if ((int)c <= (int)stop_at) f.add(cube_d2(lo, side, v, 1), v);
      }
  return f.result();
}

}  // namespace geometry
}  // namespace se

#endif /* SE_HIP_CLEARANCE_HPP */
