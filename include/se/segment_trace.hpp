/*
 * Exact segment traces on the host se::Octree snapshot that DenseSLAMSystem::getMap() materialises: the executable definition of
 * se_hip_trace_segments (include/se_hip.h), without Eigen, beside motion_collision.hpp.
 *
 * A segment runs from a to b, both in sub-units of 1 / 16 voxel (segment_sub); d = b - a, P(t) = a + t d for t in [0, 1].  A cube with
 * integer corner c and side s (voxels) is *touched* iff some t in [0, 1] has 16 c_k < a_k + t d_k < 16 (c_k + s) on every axis k: the
 * motion rule for a box of side 0, open inequalities.  An axis with d_k = 0 gives a static condition, every other axis the open interval
 *     d_k > 0:  ((16 c_k - a_k) / d_k, (16 (c_k + s) - a_k) / d_k)        d_k < 0:  ((a_k - 16 (c_k + s)) / |d_k|, (a_k - 16 c_k) / |d_k|).
 * With L the largest lower end and U the smallest upper end the cube is touched iff L < U, L < 1 and U > 0; here L is kept from 0 / 1 upwards
 * and U from 1 / 1 downwards, so that the three conditions are the one comparison L < U, and L is the entry parameter t_in.  A segment with
 * d_k = 0 and a_k a multiple of 16 on some axis lies in a grid plane and touches nothing.  The touched voxels of a segment have pairwise
 * distinct t_in: their order by t_in is the order of traversal.  Every comparison is a cross-multiplication in int64: with every
 * coordinate in [-2^22, 2^22] (trace_valid), numerators and denominators stay at or below 2^23 + 2^17 and products below 2^48.
 *
 * Three things are provided:
 *   trace_valid(seg)                  the bound;
 *   trace_literal(map, seg, ...)      the definition, literally: every voxel of the segment's bounding box tested by the predicate, the
 *                                     touched ones sorted by t_in and folded.  For short segments.  This is the model the walk and the
 *                                     device are held to;
 *   trace_walk(map, seg, ...)         what the device does: the three-axis integer DDA that advances every axis tied at the smallest
 *                                     crossing parameter, the jump to the volume's entry parameter, the cached octant (a block, or an
 *                                     absent octant with the one class all its voxels read) and, with count == false, the jump to an
 *                                     absent octant's exit parameter.  A jump lands in the voxel that holds P(t + eps): per axis the floor
 *                                     of the exact position, and on a grid plane the voxel above it for d_j > 0, below it for d_j < 0.
 * Classification is that of se_hip_collide_boxes in strict mode: test(Octree::get(v)) inside [0, size)^3, unseen outside.  A voxel blocks
 * when its class is <= stop_at.  Voxels outside the volume are never counted.
 */
#ifndef SE_HIP_SEGMENT_TRACE_HPP
#define SE_HIP_SEGMENT_TRACE_HPP

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "motion_collision.hpp"
#include "octree.hpp"
#include "octree_collision.hpp"

namespace se {
namespace geometry {

constexpr int segment_sub = 16;           /* sub-units per voxel: SE_HIP_ORIENTED_SUB */
constexpr int segment_limit = 1 << 22;    /* |coordinate| bound of a valid segment: SE_HIP_SEGMENT_LIMIT */
constexpr int trace_none = INT32_MIN;     /* first, where nothing blocks */

struct trace_result {
  bool valid;
  collision_status status;   /* meaningless when !valid (the C ABI reports SE_HIP_COLLISION_INVALID) */
  rational t_first;          /* lowest terms; motion_free, motion_invalid */
  int first[3];              /* the blocking voxel, or trace_none three times */
  int unseen, empty;         /* the counts; -1, -1 when !valid */
};

inline bool trace_valid(const int32_t seg[6]) {
  for (int k = 0; k < 6; ++k)
    if (seg[k] < -segment_limit || seg[k] > segment_limit) return false;
  return true;
}

/* the segment lies in a grid plane */
inline bool trace_degenerate(const int32_t seg[6]) {
  for (int k = 0; k < 3; ++k)
    if (seg[k] == seg[3 + k] && seg[k] % segment_sub == 0) return true;
  return false;
}

namespace trace_detail {

/* The exact predicate for the cube (corner c, side s, voxels): false iff not touched; else L (the entry parameter) and U, not reduced. */
inline bool cube(const int32_t seg[6], const int c[3], const int s, rational* Lout, rational* Uout) {
  rational L = {0, 1}, U = {1, 1};
  for (int k = 0; k < 3; ++k) {
    const int64_t a = seg[k], d = (int64_t)seg[3 + k] - seg[k], lo = (int64_t)segment_sub * c[k], hi = (int64_t)segment_sub * ((int64_t)c[k] + s);
    if (d == 0) {
      if (!(lo < a && a < hi)) return false;
      continue;
    }
    const rational lower = {d > 0 ? lo - a : a - hi, d > 0 ? d : -d};
    const rational upper = {d > 0 ? hi - a : a - lo, lower.den};
    if (L < lower) L = lower;
    if (upper < U) U = upper;
  }
  if (Lout) *Lout = L;
  if (Uout) *Uout = U;
  return L < U;
}

/* the voxel that holds P(t + eps) */
inline void land(const int32_t seg[6], const rational& t, int v[3]) {
  for (int k = 0; k < 3; ++k) {
    const int64_t a = seg[k], d = (int64_t)seg[3 + k] - seg[k];
    const int64_t p = a * t.den + t.num * d, q = (int64_t)segment_sub * t.den;
    int64_t f = p / q, r = p % q;
    if (r < 0) { --f; r += q; }
    v[k] = (int)((r == 0 && d < 0) ? f - 1 : f);
  }
}

struct fold {
  collision_status stop_at;
  trace_result r;
  explicit fold(collision_status stop) : stop_at(stop) {
    r.valid = true; r.status = collision_status::empty; r.t_first = motion_free;
    r.first[0] = r.first[1] = r.first[2] = trace_none;
    r.unseen = r.empty = 0;
  }
  /* a touched voxel, in traversal order; true: it blocks */
  bool add(const collision_status c, const bool inside, const rational& t_in, const int v[3]) {
    r.status = update_status(r.status, c);
    if ((int)c <= (int)stop_at) {
      r.t_first = lowest_terms(t_in);
      r.first[0] = v[0]; r.first[1] = v[1]; r.first[2] = v[2];
      return true;
    }
    if (inside) { if (c == collision_status::unseen) ++r.unseen; else ++r.empty; }
    return false;
  }
};

inline trace_result invalid_result() {
  trace_result r;
  r.valid = false; r.status = collision_status::empty; r.t_first = motion_invalid;
  r.first[0] = r.first[1] = r.first[2] = trace_none;
  r.unseen = r.empty = -1;
  return r;
}

inline bool in_volume(const int size, const int v[3]) { return v[0] >= 0 && v[1] >= 0 && v[2] >= 0 && v[0] < size && v[1] < size && v[2] < size; }

}  // namespace trace_detail

/* The definition: every voxel of the bounding box of the segment, each with the predicate and Octree::get, in the order of t_in. */
template <typename T, typename TestF>
trace_result trace_literal(const Octree<T>& map, const int32_t seg[6], TestF test, const collision_status stop_at) {
  if (!trace_valid(seg)) return trace_detail::invalid_result();
  auto floor16 = [](int v) { return v >= 0 ? v / segment_sub : -((-v + segment_sub - 1) / segment_sub); };
  int b0[3], b1[3];
  for (int k = 0; k < 3; ++k) {
    b0[k] = floor16(std::min(seg[k], seg[3 + k]));
    b1[k] = floor16(std::max(seg[k], seg[3 + k]));
  }
  struct entry { rational t; int v[3]; };
  std::vector<entry> touched;
  for (int z = b0[2]; z <= b1[2]; ++z)
    for (int y = b0[1]; y <= b1[1]; ++y)
      for (int x = b0[0]; x <= b1[0]; ++x) {
        entry e;
        e.v[0] = x; e.v[1] = y; e.v[2] = z;
        if (trace_detail::cube(seg, e.v, 1, &e.t, nullptr)) touched.push_back(e);
      }
  std::sort(touched.begin(), touched.end(), [](const entry& p, const entry& q) { return p.t < q.t; });
  trace_detail::fold f(stop_at);
  for (const entry& e : touched) {
    const bool in = trace_detail::in_volume(map.size(), e.v);
    if (f.add(in ? test(map.get(e.v[0], e.v[1], e.v[2])) : collision_status::unseen, in, e.t, e.v)) break;
  }
  return f.r;
}

/* The walk: what the device does.  count == false leaves a non-blocking absent octant by a jump (the counts are then not formed: 0, 0). */
template <typename T, typename TestF>
trace_result trace_walk(const Octree<T>& map, const int32_t seg[6], TestF test, const collision_status stop_at, const bool count = true) {
  using namespace trace_detail;
  if (!trace_valid(seg)) return invalid_result();
  fold f(stop_at);
  if (trace_degenerate(seg)) return f.r;
  const int size = map.size();
  int64_t d[3], ad[3];
  for (int k = 0; k < 3; ++k) { d[k] = (int64_t)seg[3 + k] - seg[k]; ad[k] = d[k] < 0 ? -d[k] : d[k]; }
  rational t = {0, 1};
  int v[3];
  land(seg, t, v);
  bool entered = false;
  /* the cached octant: corner, side; a block, or absent with the class of all its voxels */
  int oc[3] = {0, 0, 0}, os = 0;
  const VoxelBlock<T>* block = nullptr;
  collision_status ocls = collision_status::empty;
  const int origin[3] = {0, 0, 0};
  for (long left = 3l * size + 8; left > 0; --left) {
    bool jumped = false;
    if (!in_volume(size, v)) {
      if (f.add(collision_status::unseen, false, t, v) || entered) break;
      rational L;
      if (!cube(seg, origin, size, &L, nullptr)) break;   /* never enters the volume */
      t = L; jumped = true;
      entered = true;
    } else {
      entered = true;
      if (os == 0 || v[0] < oc[0] || v[0] >= oc[0] + os || v[1] < oc[1] || v[1] >= oc[1] + os || v[2] < oc[2] || v[2] >= oc[2] + os) {
        Node<T>* n = map.root();
        block = nullptr;
        os = size;
        ocls = test(voxel_traits<T>::initValue());   /* Octree::get without a root */
        if (n) {
          unsigned edge = (unsigned)size / 2;
          for (; edge >= Octree<T>::blockSide; edge /= 2) {
            const int id = ((v[0] & edge) > 0) + 2 * ((v[1] & edge) > 0) + 4 * ((v[2] & edge) > 0);
            Node<T>* child = n->child(id);
            if (!child) { ocls = test(n->value_[id]); break; }
            n = child;
          }
          if (edge < Octree<T>::blockSide) { block = static_cast<const VoxelBlock<T>*>(n); os = (int)Octree<T>::blockSide; }
          else os = (int)edge;
        }
        for (int k = 0; k < 3; ++k) oc[k] = v[k] & ~(os - 1);
      }
      const collision_status c = block ? test(block->data(v[0], v[1], v[2])) : ocls;
      if (f.add(c, true, t, v)) break;
      if (!count && !block) {
        rational U = {1, 1};
        cube(seg, oc, os, nullptr, &U);   /* (touched: the current voxel lies in it) */
        if (!(U < rational{1, 1})) break;   /* the segment ends inside the octant */
        t = U; jumped = true;
      }
    }
    if (jumped) { land(seg, t, v); continue; }
    /* a step: the smallest crossing parameter, every axis tied at it */
    rational next[3];
    bool any = false;
    rational m = {2, 1};
    for (int k = 0; k < 3; ++k) {
      if (d[k] == 0) continue;
      next[k] = rational{d[k] > 0 ? (int64_t)segment_sub * (v[k] + 1) - seg[k] : (int64_t)seg[k] - (int64_t)segment_sub * v[k], ad[k]};
      if (!any || next[k] < m) m = next[k];
      any = true;
    }
    if (!any || !(m < rational{1, 1})) break;
    for (int k = 0; k < 3; ++k)
      if (d[k] != 0 && next[k] == m) v[k] += d[k] > 0 ? 1 : -1;
    t = m;
  }
  if (!count) f.r.unseen = f.r.empty = 0;
  return f.r;
}

}  // namespace geometry
}  // namespace se

#endif /* SE_HIP_SEGMENT_TRACE_HPP */
