/*
 * Collision queries for oriented boxes, on the host se::Octree snapshot that DenseSLAMSystem::getMap() materialises: the executable
 * definition of se_hip_collide_oriented (include/se_hip.h), without Eigen, beside octree_collision.hpp and motion_collision.hpp.
 *
 * A box is a centre c and three half-axes h0, h1, h2 in sub-units of 1 / oriented_sub voxel: the open set
 * {c + s0 h0 + s1 h1 + s2 h2 : |s_i| < 1}.  The half-axes need not be orthogonal.  A cube with integer corner v and side s (voxels) is
 * *touched* iff none of 15 integer axes separates it from the box.  In doubled sub-units m = 32 v + 16 s - 2 c is the offset from the box
 * centre to the cube centre and e = 16 s the cube's half-side; an axis a separates iff
 *     a != 0   and   |a . m| >= 2 sum_i |a . h_i| + e sum_k |a_k|.
 * The axes are e_x, e_y, e_z, then h1 x h2, h2 x h0, h0 x h1, then h_i x e_k.  The inequalities are open: a face, an edge or a vertex that
 * only meets a voxel's boundary touches nothing.  Everything is int64: with |c_k| <= 2^20, |h_ik| <= 2^14 (oriented_valid) and sizes up to
 * 8192, |a_k| <= 2^29, |a . m| < 2^53 and the right-hand side < 2^49 (the arithmetic is in include/se_hip.h).
 *
 * Three things are provided:
 *   oriented_touched(box, v, s)          the exact predicate;
 *   oriented_status(map, box, test)      a plain recursive traversal of the octree, the volume's outside in closed form;
 *   oriented_status_brute(map, ...)      the definition, literally: every voxel of the box's bounding box.  This is the model the traversal
 *                                        and the device are held to.
 * Classification is that of se_hip_collide_boxes in strict mode: test(Octree::get(v)) inside [0, size)^3, unseen outside.
 */
#ifndef SE_HIP_ORIENTED_COLLISION_HPP
#define SE_HIP_ORIENTED_COLLISION_HPP

#include <cmath>
#include <cstdint>

#include "octree.hpp"
#include "octree_collision.hpp"

namespace se {
namespace geometry {

constexpr int oriented_sub = 16;                 /* sub-units per voxel: SE_HIP_ORIENTED_SUB */
constexpr int oriented_centre_limit = 1 << 20;   /* |c_k| bound of a valid box, sub-units */
constexpr int oriented_axis_limit = 1 << 14;     /* |h_ik| bound of a valid box, sub-units */

/* centre, then the three half-axes, in sub-units: the twelve int32 of the C ABI in order */
struct oriented_box {
  int32_t c[3];
  int32_t h[3][3];
};

struct oriented_result {
  collision_status status;   /* meaningless when !valid (the C ABI reports SE_HIP_COLLISION_INVALID) */
  bool valid;
};

inline oriented_box oriented_box_from(const int32_t* b) {
  oriented_box r;
  for (int k = 0; k < 3; ++k) r.c[k] = b[k];
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) r.h[i][k] = b[3 + 3 * i + k];
  return r;
}

/* The rounding helper: centre (metres), rotation (row-major 3 x 3, box frame to world: column i is the direction of box axis i) and half
 * extents (metres) of a box in a volume of `size` voxels over `dim` metres, each vector rounded to the nearest sub-unit.  The query is
 * exact for the rounded box, which lies within sqrt(3) / 8 voxel of the one asked for. */
inline oriented_box oriented_box_round(const float centre_m[3], const float rotation[9], const float half_extents_m[3], const float dim, const int size) {
  const double scale = (double)oriented_sub * size / dim;
  oriented_box r;
  for (int k = 0; k < 3; ++k) r.c[k] = (int32_t)std::nearbyint(centre_m[k] * scale);
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) r.h[i][k] = (int32_t)std::nearbyint((double)rotation[3 * k + i] * half_extents_m[i] * scale);
  return r;
}

inline int64_t oriented_det(const oriented_box& b) {
  const int64_t h00 = b.h[0][0], h01 = b.h[0][1], h02 = b.h[0][2], h10 = b.h[1][0], h11 = b.h[1][1], h12 = b.h[1][2], h20 = b.h[2][0], h21 = b.h[2][1],
                h22 = b.h[2][2];
  return h00 * (h11 * h22 - h12 * h21) + h01 * (h12 * h20 - h10 * h22) + h02 * (h10 * h21 - h11 * h20);
}

inline bool oriented_valid(const oriented_box& b) {
  for (int k = 0; k < 3; ++k) {
    if ((int64_t)b.c[k] < -oriented_centre_limit || b.c[k] > oriented_centre_limit) return false;
    for (int i = 0; i < 3; ++i)
      if ((int64_t)b.h[i][k] < -oriented_axis_limit || b.h[i][k] > oriented_axis_limit) return false;
  }
  return oriented_det(b) != 0;
}

namespace oriented_detail {

inline int64_t abs64(const int64_t v) { return v < 0 ? -v : v; }

/* does the axis a separate the cube (corner v, side s) from the valid box b? */
inline bool separates(const oriented_box& b, const int64_t a[3], const int v[3], const int s) {
  if (a[0] == 0 && a[1] == 0 && a[2] == 0) return false;
  int64_t am = 0, rb = 0, rc = 0;
  for (int k = 0; k < 3; ++k) {
    am += a[k] * (32 * (int64_t)v[k] + 16 * (int64_t)s - 2 * (int64_t)b.c[k]);
    rc += abs64(a[k]);
  }
  for (int i = 0; i < 3; ++i) rb += abs64(a[0] * b.h[i][0] + a[1] * b.h[i][1] + a[2] * b.h[i][2]);
  return abs64(am) >= 2 * rb + 16 * (int64_t)s * rc;
}

inline void cross(const int64_t u[3], const int64_t w[3], int64_t a[3]) {
  a[0] = u[1] * w[2] - u[2] * w[1];
  a[1] = u[2] * w[0] - u[0] * w[2];
  a[2] = u[0] * w[1] - u[1] * w[0];
}

}  // namespace oriented_detail

/* The exact predicate (for a valid box): is the cube with corner (x, y, z) and side s, in voxels, touched? */
inline bool oriented_touched(const oriented_box& b, const int x, const int y, const int z, const int s) {
  using namespace oriented_detail;
  const int v[3] = {x, y, z};
  int64_t h[3][3], a[3];
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) h[i][k] = b.h[i][k];
  for (int k = 0; k < 3; ++k) {
    const int64_t e[3] = {k == 0, k == 1, k == 2};
    if (separates(b, e, v, s)) return false;
  }
  for (int i = 0; i < 3; ++i) {
    cross(h[(i + 1) % 3], h[(i + 2) % 3], a);
    if (separates(b, a, v, s)) return false;
  }
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) {
      const int64_t e[3] = {k == 0, k == 1, k == 2};
      cross(h[i], e, a);
      if (separates(b, a, v, s)) return false;
    }
  return true;
}

namespace oriented_detail {

/* the box spans the open interval (c_k - ext_k, c_k + ext_k) on axis k */
inline int64_t extent(const oriented_box& b, const int k) { return abs64(b.h[0][k]) + abs64(b.h[1][k]) + abs64(b.h[2][k]); }

template <typename T, typename TestF>
void descend(Node<T>* node, const int x, const int y, const int z, const int s, const oriented_box& b, TestF test, collision_status& status) {
  const int h = s / 2;
  for (int i = 0; i < 8; ++i) {
    if (status == collision_status::occupied) return;   /* nothing beats occupied */
    const int cx = x + ((i & 1) ? h : 0), cy = y + ((i & 2) ? h : 0), cz = z + ((i & 4) ? h : 0);
    if (!oriented_touched(b, cx, cy, cz, h)) continue;
    Node<T>* child = node->child(i);
    if (!child) {
      status = update_status(status, test(node->value_[i]));   /* every voxel of the octant reads this value (Octree::get) */
    } else if (child->isLeaf()) {
      const VoxelBlock<T>* bl = static_cast<const VoxelBlock<T>*>(child);
      for (int vz = cz; vz < cz + h; ++vz)
        for (int vy = cy; vy < cy + h; ++vy)
          for (int vx = cx; vx < cx + h; ++vx)
            if (oriented_touched(b, vx, vy, vz, 1)) status = update_status(status, test(bl->data(vx, vy, vz)));
    } else {
      descend(child, cx, cy, cz, h, b, test, status);
    }
  }
}

}  // namespace oriented_detail

/* The traversal: the status of one box against the whole map. */
template <typename T, typename TestF>
oriented_result oriented_status(const Octree<T>& map, const oriented_box& b, TestF test) {
  if (!oriented_valid(b)) return {collision_status::empty, false};
  collision_status status = collision_status::empty;
  const int64_t lim = (int64_t)oriented_sub * map.size();
  for (int k = 0; k < 3; ++k) {
    const int64_t ext = oriented_detail::extent(b, k);
    if (b.c[k] - ext < 0 || b.c[k] + ext > lim) status = collision_status::unseen;   /* touches a voxel outside the volume */
  }
  if (oriented_touched(b, 0, 0, 0, map.size())) {
    if (!map.root()) status = update_status(status, test(voxel_traits<T>::initValue()));   /* Octree::get without a root */
    else oriented_detail::descend(map.root(), 0, 0, 0, map.size(), b, test, status);
  }
  return {status, true};
}

/* The definition: every voxel of the bounding box of the box, each with the predicate and Octree::get. */
template <typename T, typename TestF>
oriented_result oriented_status_brute(const Octree<T>& map, const oriented_box& b, TestF test) {
  if (!oriented_valid(b)) return {collision_status::empty, false};
  collision_status status = collision_status::empty;
  int lo[3], hi[3];
  for (int k = 0; k < 3; ++k) {
    const int64_t ext = oriented_detail::extent(b, k);
    lo[k] = (int)std::floor((double)(b.c[k] - ext) / oriented_sub) - 1;   /* (a voxel of margin: the predicate decides) */
    hi[k] = (int)std::ceil((double)(b.c[k] + ext) / oriented_sub) + 1;
  }
  const int n = map.size();
  for (int z = lo[2]; z < hi[2]; ++z)
    for (int y = lo[1]; y < hi[1]; ++y)
      for (int x = lo[0]; x < hi[0]; ++x) {
        if (!oriented_touched(b, x, y, z, 1)) continue;
        const bool in = x >= 0 && y >= 0 && z >= 0 && x < n && y < n && z < n;
        status = update_status(status, in ? test(map.get(x, y, z)) : collision_status::unseen);
      }
  return {status, true};
}

}  // namespace geometry
}  // namespace se

#endif /* SE_HIP_ORIENTED_COLLISION_HPP */
