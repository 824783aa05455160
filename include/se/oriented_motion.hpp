/*
 * Collision queries for oriented boxes moved along straight segments, on the host se::Octree snapshot that DenseSLAMSystem::getMap()
 * materialises: the executable definition of se_hip_collide_oriented_motions (include/se_hip.h), without Eigen, beside
 * oriented_collision.hpp and motion_collision.hpp.
 *
 * A motion is an oriented box (centre c, half-axes h0, h1, h2, sub-units of 1 / oriented_sub voxel) and a displacement d: at t in [0, 1] the
 * box is the open set B(t) = {c + t d + s0 h0 + s1 h1 + s2 h2 : |s_i| < 1}.  A cube with integer corner v and side s (voxels) is *touched*
 * iff some t in [0, 1] has B(t) touching it as oriented_touched defines it.  Per axis a of that test (e_k, h_i x h_j, h_i x e_k; a zero axis
 * takes no part), in doubled sub-units:
 *     m = 32 v + 16 s - 2 c,   p = a . m,   q = 2 (a . d),   R = 2 sum_i |a . h_i| + 16 s sum_k |a_k|,
 * and the box at t is not separated by a iff |p - t q| < R: an axis with q = 0 gives the static condition |p| < R, every other axis the open
 * interval ((p' - R) / |q|, (p' + R) / |q|) with p' = p sign(q).  With L the largest lower end and U the smallest upper end the cube is
 * touched iff every static condition holds and L < U, L < 1, U > 0, and its entry parameter is t_in = max(0, L).  Here L and U are kept
 * already clamped -- L from 0 / 1 upwards, U from 1 / 1 downwards -- so that the three conditions are the one comparison L < U.  t_in is an
 * infimum: a vertex that only meets a voxel's corner at t = 0 and then slides into the voxel gives t_in = 0.
 * With |c_k|, |c_k + d_k| <= 2^20, |h_ik| <= 2^14, |d_k| <= 2^18 (oriented_motion_valid) and sizes up to 8192: |p| < 2^53, |q| < 2^50,
 * R < 2^49, numerators below 2^54 -- int64, and two rationals are compared by cross-multiplication in __int128 (the arithmetic is in
 * include/se_hip.h).
 *
 * The swept set is also the open zonotope with generators h0, h1, h2, d / 2 about c + d / 2: oriented_motion_swept states the 21-axis
 * separating test of that form, which the device uses to decide *touched*; the tests hold the two forms together.
 *
 * Provided:
 *   oriented_motion_entry(box, d, v, s, &t_in)     the exact predicate and the entry parameter (not reduced);
 *   oriented_motion_swept(box, d, v, s)            the 21-axis form of the predicate;
 *   oriented_motion_status(map, motion, ...)       a plain recursive traversal of the octree, the volume's outside in closed form;
 *   oriented_motion_status_brute(map, ...)         the definition, literally: every voxel of the bounding box of the sweep.  This is the model
 *                                                  the traversal and the device are held to;
 *   oriented_motion_round(...)                     a motion from a metric centre, rotation, half extents and displacement.
 * Classification is that of se_hip_collide_boxes in strict mode: test(Octree::get(v)) inside [0, size)^3, unseen outside.  A voxel blocks
 * when its class is <= stop_at; t_exact is the smallest t_in over the touched blocking voxels.
 */
#ifndef SE_HIP_ORIENTED_MOTION_HPP
#define SE_HIP_ORIENTED_MOTION_HPP

#include <cmath>
#include <cstdint>

#include "motion_collision.hpp"
#include "octree.hpp"
#include "octree_collision.hpp"
#include "oriented_collision.hpp"

namespace se {
namespace geometry {

constexpr int oriented_move_limit = 1 << 18;   /* |d_k| bound of a valid motion, sub-units: SE_HIP_ORIENTED_MOVE_LIMIT */

/* the fifteen int32 of the C ABI in order: the box, then the displacement */
struct oriented_motion {
  oriented_box box;
  int32_t d[3];
};

struct oriented_motion_result {
  collision_status status;   /* meaningless when !valid (the C ABI reports SE_HIP_COLLISION_INVALID) */
  rational t_exact;          /* lowest terms; motion_free, motion_invalid */
  bool valid;
};

inline oriented_motion oriented_motion_from(const int32_t* m) {
  oriented_motion r;
  r.box = oriented_box_from(m);
  for (int k = 0; k < 3; ++k) r.d[k] = m[12 + k];
  return r;
}

/* The rounding helper: oriented_box_round for the box, the displacement (metres) rounded to the nearest sub-unit like the centre.  The
 * query is exact for the rounded motion. */
inline oriented_motion oriented_motion_round(const float centre_m[3], const float rotation[9], const float half_extents_m[3], const float displacement_m[3],
                                             const float dim, const int size) {
  const double scale = (double)oriented_sub * size / dim;
  oriented_motion r;
  r.box = oriented_box_round(centre_m, rotation, half_extents_m, dim, size);
  for (int k = 0; k < 3; ++k) r.d[k] = (int32_t)std::nearbyint(displacement_m[k] * scale);
  return r;
}

inline bool oriented_motion_valid(const oriented_motion& m) {
  if (!oriented_valid(m.box)) return false;
  for (int k = 0; k < 3; ++k) {
    const int64_t d = m.d[k], e = (int64_t)m.box.c[k] + d;
    if (d < -oriented_move_limit || d > oriented_move_limit || e < -oriented_centre_limit || e > oriented_centre_limit) return false;
  }
  return true;
}

/* the float the C ABI returns for a reduced pair */
inline float oriented_motion_float(const rational& r) { return (float)((double)r.num / (double)r.den); }

namespace oriented_motion_detail {

using oriented_detail::abs64;
using oriented_detail::cross;

/* a < b for terms up to 2^54 (motion_collision.hpp's operator< multiplies in int64) */
inline bool less(const rational& a, const rational& b) { return (__int128)a.num * b.den < (__int128)b.num * a.den; }

/* one axis of the interval form: false iff it does not move and separates; else its interval is folded into L (from below) and U (from above) */
inline bool interval(const oriented_box& b, const int32_t d[3], const int64_t a[3], const int v[3], const int s, rational& L, rational& U) {
  if (a[0] == 0 && a[1] == 0 && a[2] == 0) return true;
  int64_t p = 0, q = 0, rb = 0, rc = 0;
  for (int k = 0; k < 3; ++k) {
    p += a[k] * (32 * (int64_t)v[k] + 16 * (int64_t)s - 2 * (int64_t)b.c[k]);
    q += 2 * a[k] * d[k];
    rc += abs64(a[k]);
  }
  for (int i = 0; i < 3; ++i) rb += abs64(a[0] * b.h[i][0] + a[1] * b.h[i][1] + a[2] * b.h[i][2]);
  const int64_t R = 2 * rb + 16 * (int64_t)s * rc;
  if (q == 0) return abs64(p) < R;
  const int64_t pp = q > 0 ? p : -p, aq = abs64(q);
  const rational lower = {pp - R, aq}, upper = {pp + R, aq};
  if (less(L, lower)) L = lower;
  if (less(upper, U)) U = upper;
  return true;
}

/* does the axis a separate the cube from the swept zonotope? */
inline bool separates_swept(const oriented_box& b, const int32_t d[3], const int64_t a[3], const int v[3], const int s) {
  if (a[0] == 0 && a[1] == 0 && a[2] == 0) return false;
  int64_t am = 0, ad = 0, rb = 0, rc = 0;
  for (int k = 0; k < 3; ++k) {
    am += a[k] * (32 * (int64_t)v[k] + 16 * (int64_t)s - 2 * (int64_t)b.c[k] - d[k]);
    ad += a[k] * d[k];
    rc += abs64(a[k]);
  }
  for (int i = 0; i < 3; ++i) rb += abs64(a[0] * b.h[i][0] + a[1] * b.h[i][1] + a[2] * b.h[i][2]);
  return abs64(am) >= 2 * rb + abs64(ad) + 16 * (int64_t)s * rc;
}

}  // namespace oriented_motion_detail

/* The exact predicate, by the interval form (for a valid motion): is the cube with corner v and side s, in voxels, touched, and if so at
 * which parameter first (not reduced)? */
inline bool oriented_motion_entry(const oriented_box& b, const int32_t d[3], const int v[3], const int s, rational* t_in) {
  using namespace oriented_motion_detail;
  rational L = {0, 1}, U = {1, 1};
  int64_t h[3][3], a[3];
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) h[i][k] = b.h[i][k];
  for (int k = 0; k < 3; ++k) {
    const int64_t e[3] = {k == 0, k == 1, k == 2};
    if (!interval(b, d, e, v, s, L, U)) return false;
  }
  for (int i = 0; i < 3; ++i) {
    cross(h[(i + 1) % 3], h[(i + 2) % 3], a);
    if (!interval(b, d, a, v, s, L, U)) return false;
  }
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) {
      const int64_t e[3] = {k == 0, k == 1, k == 2};
      cross(h[i], e, a);
      if (!interval(b, d, a, v, s, L, U)) return false;
    }
  if (!less(L, U)) return false;
  if (t_in) *t_in = L;
  return true;
}

/* The same predicate by the 21-axis form: no axis separates the cube from the open zonotope the box sweeps. */
inline bool oriented_motion_swept(const oriented_box& b, const int32_t d[3], const int v[3], const int s) {
  using namespace oriented_motion_detail;
  int64_t g[4][3], a[3];
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) g[i][k] = b.h[i][k];
  for (int k = 0; k < 3; ++k) g[3][k] = d[k];
  for (int k = 0; k < 3; ++k) {
    const int64_t e[3] = {k == 0, k == 1, k == 2};
    if (separates_swept(b, d, e, v, s)) return false;
  }
  for (int i = 0; i < 4; ++i)
    for (int j = i + 1; j < 4; ++j) {
      cross(g[i], g[j], a);
      if (separates_swept(b, d, a, v, s)) return false;
    }
  for (int i = 0; i < 4; ++i)
    for (int k = 0; k < 3; ++k) {
      const int64_t e[3] = {k == 0, k == 1, k == 2};
      cross(g[i], e, a);
      if (separates_swept(b, d, a, v, s)) return false;
    }
  return true;
}

namespace oriented_motion_detail {

struct fold {
  collision_status stop_at;
  collision_status status = collision_status::empty;
  rational best = motion_free;
  void add(const collision_status c, const rational& t_in) {
    status = update_status(status, c);
    if ((int)c <= (int)stop_at && less(t_in, best)) best = t_in;
  }
  /* nothing at or after t_in can change either output (exact: t_in of a part of a cube is never smaller than the cube's) */
  bool settled(const rational& t_in) const { return status == collision_status::occupied && !less(t_in, best); }
};

/* the part of the motion outside [0, size)^3: the touched voxels there are unseen, and per volume face the first parameter at which one of
 * them is touched has a closed form */
inline void outside(const int size, const oriented_motion& m, fold& f) {
  const int64_t lim = (int64_t)oriented_sub * size;
  for (int k = 0; k < 3; ++k) {
    const int64_t ext = oriented_detail::extent(m.box, k), lo = m.box.c[k] - ext, hi = m.box.c[k] + ext, dk = m.d[k];
    /* voxels with v_k < 0 */
    if (lo < 0) f.add(collision_status::unseen, {0, 1});
    else if (dk < 0 && lo < -dk) f.add(collision_status::unseen, {lo, -dk});
    /* voxels with v_k >= size */
    if (hi > lim) f.add(collision_status::unseen, {0, 1});
    else if (dk > 0 && lim - hi < dk) f.add(collision_status::unseen, {lim - hi, dk});
  }
}

template <typename T, typename TestF>
void descend(Node<T>* node, const int x, const int y, const int z, const int s, const oriented_motion& m, TestF test, fold& f) {
  const int h = s / 2;
  for (int i = 0; i < 8; ++i) {
    const int c[3] = {x + ((i & 1) ? h : 0), y + ((i & 2) ? h : 0), z + ((i & 4) ? h : 0)};
    rational t;
    if (!oriented_motion_entry(m.box, m.d, c, h, &t) || f.settled(t)) continue;
    Node<T>* child = node->child(i);
    if (!child) {
      f.add(test(node->value_[i]), t);   /* every voxel of the octant reads this value (Octree::get) */
    } else if (child->isLeaf()) {
      const VoxelBlock<T>* bl = static_cast<const VoxelBlock<T>*>(child);
      for (int vz = c[2]; vz < c[2] + h; ++vz)
        for (int vy = c[1]; vy < c[1] + h; ++vy)
          for (int vx = c[0]; vx < c[0] + h; ++vx) {
            const int v[3] = {vx, vy, vz};
            if (oriented_motion_entry(m.box, m.d, v, 1, &t)) f.add(test(bl->data(vx, vy, vz)), t);
          }
    } else {
      descend(child, c[0], c[1], c[2], h, m, test, f);
    }
  }
}

}  // namespace oriented_motion_detail

/* The traversal: status and first blocking parameter of one motion against the whole map. */
template <typename T, typename TestF>
oriented_motion_result oriented_motion_status(const Octree<T>& map, const oriented_motion& m, TestF test, const collision_status stop_at) {
  if (!oriented_motion_valid(m)) return {collision_status::empty, motion_invalid, false};
  oriented_motion_detail::fold f;
  f.stop_at = stop_at;
  oriented_motion_detail::outside(map.size(), m, f);
  const int origin[3] = {0, 0, 0};
  rational t;
  if (oriented_motion_entry(m.box, m.d, origin, map.size(), &t)) {
    if (!map.root()) f.add(test(voxel_traits<T>::initValue()), t);   /* Octree::get without a root */
    else oriented_motion_detail::descend(map.root(), 0, 0, 0, map.size(), m, test, f);
  }
  return {f.status, lowest_terms(f.best), true};
}

/* The definition: every voxel of the bounding box of the sweep, each with the predicate and Octree::get. */
template <typename T, typename TestF>
oriented_motion_result oriented_motion_status_brute(const Octree<T>& map, const oriented_motion& m, TestF test, const collision_status stop_at) {
  if (!oriented_motion_valid(m)) return {collision_status::empty, motion_invalid, false};
  oriented_motion_detail::fold f;
  f.stop_at = stop_at;
  int lo[3], hi[3];
  for (int k = 0; k < 3; ++k) {
    const int64_t ext = oriented_detail::extent(m.box, k);
    const int64_t a = m.box.c[k] - ext + (m.d[k] < 0 ? m.d[k] : 0), b = m.box.c[k] + ext + (m.d[k] > 0 ? m.d[k] : 0);
    lo[k] = (int)std::floor((double)a / oriented_sub) - 1;   /* (a voxel of margin: the predicate decides) */
    hi[k] = (int)std::ceil((double)b / oriented_sub) + 1;
  }
  const int n = map.size();
  for (int z = lo[2]; z < hi[2]; ++z)
    for (int y = lo[1]; y < hi[1]; ++y)
      for (int x = lo[0]; x < hi[0]; ++x) {
        const int v[3] = {x, y, z};
        rational t;
        if (!oriented_motion_entry(m.box, m.d, v, 1, &t)) continue;
        const bool in = x >= 0 && y >= 0 && z >= 0 && x < n && y < n && z < n;
        f.add(in ? test(map.get(x, y, z)) : collision_status::unseen, t);
      }
  return {f.status, lowest_terms(f.best), true};
}

}  // namespace geometry
}  // namespace se

#endif /* SE_HIP_ORIENTED_MOTION_HPP */
