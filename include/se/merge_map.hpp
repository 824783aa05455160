/*
 * se::merge_map on two host se::Octree snapshots that DenseSLAMSystem::getMap() materialises (include/se/octree.hpp): the executable
 * definition of the device's se_hip_merge_map (include/se_hip.h) -- what DenseSLAMSystem::mergeMap leaves in the device map is what
 * merge_map makes of the two snapshots taken before.  The reference has no counterpart: it holds one map.
 *
 * Source content at voxel c meets destination content at c + s.  se::merge_value is the value-pair function, for block voxels and node
 * value_[j] alike (a = destination, b = source; "unseen": x == initValue().x && y == initValue().y, y compared as float):
 *     b unseen                   a stays, bit for bit, in every mode
 *     a unseen, or REPLACE       b, bit for bit; SDF: y = fminf(b.y, max_weight)
 *     FILL                       a stays
 *     FUSE, SDF                  b.y == 0: a stays; a.y == 0: as "a unseen"; else w = a.y + b.y,
 *                                x = clamp((a.y * a.x + b.y * b.x) / w, -1, 1), y = fminf(w, max_weight)
 *                                (sdf_update's running mean, kfusion/mapping_impl.hpp:56-60, the second sample weighing b.y instead of 1)
 *     FUSE, OFusion              x = clamp(a.x + b.x, BOTTOM_CLAMP, TOP_CLAMP) (+-1000, volume_traits.hpp), y = fmaxf(a.y, b.y)
 * binary32 in that order, no contraction (build with -ffp-contract=off), IEEE division; clamp(v, lo, hi) = std::max(lo, std::min(v, hi)).
 *
 *   arguments  merge_valid: both trees distinct, dim / size (a binary32 division) bit-equal, every component of s a multiple of 8 within
 *              [-2^30, 2^30], a known mode, max_weight an integer in [1, 255]; anything else leaves both maps untouched (counts all -1).
 *              The sizes may differ.
 *   blocks     the source block with corner c takes part iff c + s lies in [0, dst size - 8] on every axis, else it is clipped.  Its block
 *              in dst is created if absent, with all missing ancestors and initValue() (Octree::allocate, allocate_region.hpp: without the
 *              keys[0] rule); the 512 values are combined; active_ = the OR of the two flags, a created block is active
 *   nodes      the source node of side d (level >= 1, childless ones included) and corner c takes part iff every component of s is a
 *              multiple of d and c + s lies in [0, dst size - d]; its level in dst is the one of side d.  It is created if absent and its
 *              value_[8] are combined.  Any other source node is skipped.  The source root takes part only if s == 0 and the sizes are
 *              equal.  A source node value is never pushed down into destination voxels
 *   counts     (optional, int64[12]) blocks combined, blocks created, source blocks clipped, nodes combined, nodes created for source nodes,
 *              source nodes skipped, lo[3] and hi[3] of the destination voxel box of the blocks that took part (half open, zero if none)
 * The destination's buffers are in key order afterwards, as getMap() delivers them, and the tree is linked.  The source is only read.
 */
#ifndef SE_HIP_MERGE_MAP_HPP
#define SE_HIP_MERGE_MAP_HPP

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <set>
#include <type_traits>

#include "allocate_region.hpp"
#include "octree.hpp"
#include "shift_map.hpp"

namespace se {

enum { MERGE_FUSE = 0, MERGE_REPLACE = 1, MERGE_FILL = 2 };   /* SE_HIP_MERGE_* */
struct merge_rule { int mode = MERGE_FUSE; float max_weight = 100.f; };

namespace merge_detail {
inline float clamp(float v, float lo, float hi) { return std::max(lo, std::min(v, hi)); }
}  // namespace merge_detail

template <typename T>
inline typename voxel_traits<T>::value_type merge_value(typename voxel_traits<T>::value_type a, typename voxel_traits<T>::value_type b, int mode, float max_weight) {
  typedef typename voxel_traits<T>::value_type value_type;
  const bool sdf = std::is_same<T, SDF>::value;
  const value_type init = voxel_traits<T>::initValue();
  const float ix = init.x, iy = (float)init.y;
  const float ax = a.x, ay = (float)a.y, bx = b.x, by = (float)b.y;
  if (bx == ix && by == iy) return a;
  value_type taken = b;
  if (sdf) taken.y = fminf(by, max_weight);
  if ((ax == ix && ay == iy) || mode == MERGE_REPLACE) return taken;
  if (mode == MERGE_FILL) return a;
  value_type out = a;
  if (!sdf) {
    out.x = merge_detail::clamp(ax + bx, -1000.f, 1000.f);
    out.y = fmaxf(ay, by);
    return out;
  }
  if (by == 0.f) return a;
  if (ay == 0.f) return taken;
  const float w = ay + by;
  out.x = merge_detail::clamp((ay * ax + by * bx) / w, -1.f, 1.f);
  out.y = fminf(w, max_weight);
  return out;
}

template <typename T>
bool merge_valid(const Octree<T>& dst, const Octree<T>& src, const int s[3], const merge_rule& rule) {
  if (&dst == &src || dst.size() <= 0 || src.size() <= 0) return false;
  const float va = dst.dim() / (float)dst.size(), vb = src.dim() / (float)src.size();
  if (std::memcmp(&va, &vb, sizeof va) != 0) return false;
  if (!shift_valid(s)) return false;
  if (rule.mode != MERGE_FUSE && rule.mode != MERGE_REPLACE && rule.mode != MERGE_FILL) return false;
  return rule.max_weight >= 1.f && rule.max_weight <= 255.f && rule.max_weight == (float)(int)rule.max_weight;
}

template <typename T>
void merge_map(Octree<T>& dst, Octree<T>& src, const int s[3], const merge_rule& rule = merge_rule(), int64_t* counts = nullptr) {
  if (!merge_valid(dst, src, s, rule)) {
    if (counts) for (int k = 0; k < 12; ++k) counts[k] = -1;
    return;
  }
  const int size = dst.size();
  int max_level = 0;
  for (int v = size; v > 1; v >>= 1) ++max_level;
  const int leaf_level = max_level - 3;
  auto& nodes = dst.getNodesBuffer();
  auto& blocks = dst.getBlockBuffer();
  std::map<key_t, Node<T>*> have_n;
  std::map<key_t, VoxelBlock<T>*> have_b;
  for (auto& n : nodes) have_n[n->code_] = n.get();
  for (auto& b : blocks) have_b[b->code_] = b.get();
  if (!have_n.count(0)) have_n[0] = dst.add_node(0, (unsigned)size);   /* (a snapshot always holds the root) */
  std::set<key_t> before;   /* "existed" means before the call: a node created as another's ancestor on the way does not count as found */
  for (auto& kv : have_n) before.insert(kv.first);
  int64_t c[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const bool zero = s[0] == 0 && s[1] == 0 && s[2] == 0;
  /* does the source octant with side d and corner p take part?  q = its corner in dst */
  auto moved = [&](const int p[3], int d, int q[3]) {
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
      ok = ok && s[k] % d == 0;
      const long v = (long)p[k] + (long)s[k];
      ok = ok && v >= 0 && v <= (long)size - d;
      q[k] = (int)v;
    }
    return ok;
  };
  /* every missing ancestor of the octant with corner q at `level`, with initValue() */
  auto ancestors = [&](const int q[3], int level) {
    for (int l = level - 1; l >= 1; --l) {
      const int d = size >> l;
      const key_t up = alloc_detail::make_key(q[0] / d * d, q[1] / d * d, q[2] / d * d, l);
      if (have_n.count(up)) break;   /* the first that exists has all of its own */
      have_n[up] = dst.add_node(up, (unsigned)d);
    }
  };
  for (auto& n : src.getNodesBuffer()) {
    const int slevel = (int)(n->code_ & 0x1FFull);
    const key_t code = n->code_ & ~0x1FFull;
    const int d = src.size() >> slevel;
    const int p[3] = {shift_detail::compact21(code, 0), shift_detail::compact21(code, 1), shift_detail::compact21(code, 2)};
    int q[3];
    bool take = moved(p, d, q);
    if (slevel == 0) take = take && zero && src.size() == size;
    if (!take) { ++c[5]; continue; }
    int level = 0;
    for (int v = size; v > d; v >>= 1) ++level;
    const key_t key = alloc_detail::make_key(q[0], q[1], q[2], level);
    Node<T>* t = nullptr;
    auto it = have_n.find(key);
    if (it != have_n.end()) t = it->second;
    else { t = dst.add_node(key, (unsigned)d); have_n[key] = t; ancestors(q, level); }
    ++c[before.count(key) ? 3 : 4];
    for (int j = 0; j < 8; ++j) t->value_[j] = merge_value<T>(t->value_[j], n->value_[j], rule.mode, rule.max_weight);
  }
  bool any = false;
  for (auto& b : src.getBlockBuffer()) {
    int q[3];
    if (!moved(b->coordinates_, 8, q)) { ++c[2]; continue; }
    const key_t key = alloc_detail::make_key(q[0], q[1], q[2], leaf_level);
    VoxelBlock<T>* t = nullptr;
    auto it = have_b.find(key);
    if (it != have_b.end()) { t = it->second; ++c[0]; }
    else { t = dst.add_block(key, q, true); have_b[key] = t; ancestors(q, leaf_level); ++c[1]; }
    for (int j = 0; j < 512; ++j) t->voxel_block_[j] = merge_value<T>(t->voxel_block_[j], b->voxel_block_[j], rule.mode, rule.max_weight);
    t->active_ = t->active_ || b->active_;
    for (int k = 0; k < 3; ++k) {
      c[6 + k] = any ? std::min<int64_t>(c[6 + k], q[k]) : q[k];
      c[9 + k] = any ? std::max<int64_t>(c[9 + k], q[k] + 8) : q[k] + 8;
    }
    any = true;
  }
  auto by_key = [](const auto& p, const auto& q) { return p->code_ < q->code_; };
  std::sort(nodes.begin(), nodes.end(), by_key);
  std::sort(blocks.begin(), blocks.end(), by_key);
  dst.finalize();
  if (counts) for (int k = 0; k < 12; ++k) counts[k] = c[k];
}

}  // namespace se

#endif /* SE_HIP_MERGE_MAP_HPP */
