/*
 * Collision queries for boxes moved along straight segments, on the host se::Octree snapshot that DenseSLAMSystem::getMap() materialises:
 * the executable definition of se_hip_collide_motions (include/se_hip.h), without Eigen, beside octree_collision.hpp.
 *
 * A motion is the box [lo, lo + side) translated by t * d for t in [0, 1], everything in whole voxels.  A cube with integer corner c and
 * side s is *touched* iff some t in [0, 1] has, on every axis k,   lo_k + t d_k < c_k + s   and   lo_k + side_k + t d_k > c_k   (open).
 * An axis with d_k = 0 gives a static condition; every other axis the open interval
 *     d_k > 0:  ((c_k - side_k - lo_k) / d_k, (c_k + s - lo_k) / d_k)        d_k < 0:  ((lo_k - c_k - s) / |d_k|, (lo_k + side_k - c_k) / |d_k|)
 * which is never empty (its ends differ by (s + side_k) / |d_k|).  With L the largest lower end and U the smallest upper end the cube is
 * touched iff L < U, L < 1 and U > 0, and its entry parameter is t_in = max(0, L).  Here L and U are kept already clamped -- L from 0 / 1
 * upwards, U from 1 / 1 downwards -- so that the three conditions are the one comparison L < U.  Every comparison is a cross-multiplication
 * in int64: with lo, lo + side, lo + d, lo + side + d in [-2^20, 2^20] (motion_valid) and cubes inside that range, numerators and
 * denominators stay below 2^24 and products below 2^48.
 *
 * Three things are provided:
 *   touched(lo, side, d, c, s, &t_in)            the exact predicate;
 *   motion_status_and_entry(map, ...)            a plain recursive traversal of the octree, the volume's outside in closed form;
 *   motion_status_and_entry_brute(map, ...)      the definition, literally: every voxel of the motion's bounding box.  This is the model the
 *                                                traversal and the device are held to.
 * Classification is that of se_hip_collide_boxes in strict mode: test(Octree::get(v)) inside [0, size)^3, unseen outside.  A voxel blocks
 * when its class is <= stop_at (occupied, or unseen: unseen and occupied); t_first is the smallest t_in over the touched blocking voxels.
 */
#ifndef SE_HIP_MOTION_COLLISION_HPP
#define SE_HIP_MOTION_COLLISION_HPP

#include <cstdint>
#include <initializer_list>

#include "octree.hpp"
#include "octree_collision.hpp"

namespace se {
namespace geometry {

constexpr int motion_limit = 1 << 20;   /* |coordinate| bound of a valid motion */

/* a non-negative rational; den > 0.  Results are returned in lowest terms. */
struct rational {
  int64_t num, den;
};
inline bool operator<(const rational& a, const rational& b) { return a.num * b.den < b.num * a.den; }
inline bool operator==(const rational& a, const rational& b) { return a.num * b.den == b.num * a.den; }
inline rational lowest_terms(rational r) {
  int64_t a = r.num < 0 ? -r.num : r.num, b = r.den;
  while (b) { const int64_t t = a % b; a = b; b = t; }
  if (a > 1) { r.num /= a; r.den /= a; }
  return r;
}
/* the float the C ABI returns for it: both terms are exactly representable, so the quotient depends on the value alone */
inline float to_float(const rational& r) { return (float)r.num / (float)r.den; }

constexpr rational motion_free = {2, 1};      /* nothing blocks: SE_HIP_MOTION_FREE */
constexpr rational motion_invalid = {-1, 1};  /* t_first of an invalid motion */

struct motion_result {
  collision_status status;   /* meaningless when !valid (the C ABI reports SE_HIP_COLLISION_INVALID) */
  rational t_first;          /* lowest terms; motion_free, motion_invalid */
  bool valid;
};

template <typename Vec3i>
inline bool motion_valid(const Vec3i& lo, const Vec3i& side, const Vec3i& d) {
  for (int k = 0; k < 3; ++k) {
    const int64_t a = lo(k), b = (int64_t)lo(k) + side(k), c = (int64_t)lo(k) + d(k), e = b + d(k);
    if (side(k) < 1) return false;
    for (int64_t v : {a, b, c, e})
      if (v < -motion_limit || v > motion_limit) return false;
  }
  return true;
}

/* The exact predicate.  Returns whether the cube (corner c, side s) is touched and, if so, its entry parameter (not reduced). */
template <typename Vec3i, typename Vec3j>
inline bool touched(const Vec3i& lo, const Vec3i& side, const Vec3i& d, const Vec3j& c, const int s, rational* t_in) {
  rational L = {0, 1}, U = {1, 1};
  for (int k = 0; k < 3; ++k) {
    const int64_t l = lo(k), e = side(k), dk = d(k), ck = c(k);
    if (dk == 0) {
      if (!(l < ck + s && l + e > ck)) return false;
      continue;
    }
    const rational lower = {dk > 0 ? ck - e - l : l - ck - s, dk > 0 ? dk : -dk};
    const rational upper = {dk > 0 ? ck + s - l : l + e - ck, lower.den};
    if (L < lower) L = lower;
    if (upper < U) U = upper;
  }
  if (!(L < U)) return false;
  if (t_in) *t_in = L;
  return true;
}

namespace motion_detail {

struct fold {
  collision_status stop_at;
  collision_status status = collision_status::empty;
  rational best = motion_free;
  void add(const collision_status c, const rational& t_in) {
    status = update_status(status, c);
    if ((int)c <= (int)stop_at && t_in < best) best = t_in;
  }
  /* nothing at or after t_in can change either output (exact: t_in of a part of a cube is never smaller than the cube's) */
  bool settled(const rational& t_in) const { return status == collision_status::occupied && !(t_in < best); }
};

/* the part of the motion outside [0, size)^3: the touched voxels there are unseen, and per volume face the first parameter at which one of
 * them is touched has a closed form */
template <typename Vec3i>
inline void outside(const int size, const Vec3i& lo, const Vec3i& side, const Vec3i& d, fold& f) {
  for (int k = 0; k < 3; ++k) {
    const int64_t l = lo(k), h = (int64_t)lo(k) + side(k), dk = d(k);
    /* voxels with v_k < 0 */
    if (l < 0) f.add(collision_status::unseen, {0, 1});
    else if (dk < 0 && l < -dk) f.add(collision_status::unseen, {l, -dk});
    /* voxels with v_k >= size */
    if (h > size) f.add(collision_status::unseen, {0, 1});
    else if (dk > 0 && size - h < dk) f.add(collision_status::unseen, {size - h, dk});
  }
}

template <typename T, typename Vec3i, typename TestF>
void descend(Node<T>* node, const int x, const int y, const int z, const int s, const Vec3i& lo, const Vec3i& side, const Vec3i& d, TestF test, fold& f) {
  const int h = s / 2;
  for (int i = 0; i < 8; ++i) {
    const int3 c = {{x + ((i & 1) ? h : 0), y + ((i & 2) ? h : 0), z + ((i & 4) ? h : 0)}};
    rational t;
    if (!touched(lo, side, d, c, h, &t) || f.settled(t)) continue;
    Node<T>* child = node->child(i);
    if (!child) {
      f.add(test(node->value_[i]), t);   /* every voxel of the octant reads this value (Octree::get) */
    } else if (child->isLeaf()) {
      const VoxelBlock<T>* b = static_cast<const VoxelBlock<T>*>(child);
      for (int vz = c(2); vz < c(2) + h; ++vz)
        for (int vy = c(1); vy < c(1) + h; ++vy)
          for (int vx = c(0); vx < c(0) + h; ++vx) {
            const int3 v = {{vx, vy, vz}};
            if (touched(lo, side, d, v, 1, &t)) f.add(test(b->data(vx, vy, vz)), t);
          }
    } else {
      descend(child, c(0), c(1), c(2), h, lo, side, d, test, f);
    }
  }
}

}  // namespace motion_detail

/* The traversal: status and first blocking parameter of one motion against the whole map. */
template <typename T, typename Vec3i, typename TestF>
motion_result motion_status_and_entry(const Octree<T>& map, const Vec3i& lo, const Vec3i& side, const Vec3i& d, TestF test, const collision_status stop_at) {
  if (!motion_valid(lo, side, d)) return {collision_status::empty, motion_invalid, false};
  motion_detail::fold f;
  f.stop_at = stop_at;
  motion_detail::outside(map.size(), lo, side, d, f);
  const int3 origin = {{0, 0, 0}};
  rational t;
  if (touched(lo, side, d, origin, map.size(), &t)) {
    if (!map.root()) f.add(test(voxel_traits<T>::initValue()), t);   /* Octree::get without a root */
    else motion_detail::descend(map.root(), 0, 0, 0, map.size(), lo, side, d, test, f);
  }
  return {f.status, lowest_terms(f.best), true};
}

/* The definition: every voxel of the bounding box of the motion, each with the predicate and Octree::get. */
template <typename T, typename Vec3i, typename TestF>
motion_result motion_status_and_entry_brute(const Octree<T>& map, const Vec3i& lo, const Vec3i& side, const Vec3i& d, TestF test, const collision_status stop_at) {
  if (!motion_valid(lo, side, d)) return {collision_status::empty, motion_invalid, false};
  motion_detail::fold f;
  f.stop_at = stop_at;
  int b0[3], b1[3];
  for (int k = 0; k < 3; ++k) {
    b0[k] = lo(k) + (d(k) < 0 ? d(k) : 0);
    b1[k] = lo(k) + side(k) + (d(k) > 0 ? d(k) : 0);
  }
  const int n = map.size();
  for (int z = b0[2]; z < b1[2]; ++z)
    for (int y = b0[1]; y < b1[1]; ++y)
      for (int x = b0[0]; x < b1[0]; ++x) {
        const int3 v = {{x, y, z}};
        rational t;
        if (!touched(lo, side, d, v, 1, &t)) continue;
        const bool in = x >= 0 && y >= 0 && z >= 0 && x < n && y < n && z < n;
        f.add(in ? test(map.get(x, y, z)) : collision_status::unseen, t);
      }
  return {f.status, lowest_terms(f.best), true};
}

}  // namespace geometry
}  // namespace se

#endif /* SE_HIP_MOTION_COLLISION_HPP */
