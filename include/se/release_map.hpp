/*
 * se::release_map on the host se::Octree snapshot that DenseSLAMSystem::getMap() materialises (include/se/octree.hpp): the executable
 * definition of the device's se_hip_release_boxes (include/se_hip.h) -- what DenseSLAMSystem::releaseMap leaves in the device map is what
 * release_map makes of the snapshot taken before.  The reference has no counterpart: nothing in its octree is ever freed.
 *
 * Octants that lie wholly inside a box are handed back: every one of them (SE_HIP_RELEASE_ALL: the region is forgotten) or only those that
 * hold nothing (SE_HIP_RELEASE_UNSEEN).
 *
 *   arguments  n <= 4096; per record side >= 1, lo and lo + side within [-2^30, 2^30], what one of the two codes, reserved 0; anything else
 *              leaves the map untouched (release_boxes_valid; counts are then all -1).  n = 0 is valid and changes nothing.
 *   contains   a record contains the octant with corner c and side d iff c >= lo and c + d <= lo + side on every axis
 *   blocks     released iff some record contains the block and that record is ALL, or is UNSEEN and all 512 voxels equal initValue() in x and y
 *              bit for bit (y as the float the device holds)
 *   nodes      releasable iff some record contains the node and that record is ALL or all eight value_[i] equal initValue() bit for bit;
 *              released iff releasable and every block and node beneath it is released.  The root always stays.  An ancestor of a survivor is
 *              never released, so nothing has to be created (asserted below)
 *   parents    for every released octant whose parent stays, the parent's value_[child] becomes initValue(): Octree::get is initValue() at
 *              every voxel of a released block afterwards.  Nothing else in a survivor changes
 *   counts     (optional, int64[5]) blocks kept, blocks released, nodes kept (the root included), nodes released, released blocks that held
 *              at least one observed voxel
 *   touched    (optional, int32[6]) lo and hi of the half-open voxel box of the released blocks; all zero when none was released
 * The snapshot's buffers are in key order afterwards, as getMap() delivers them, and the tree is linked.
 */
#ifndef SE_HIP_RELEASE_MAP_HPP
#define SE_HIP_RELEASE_MAP_HPP

#include <algorithm>
#include <cassert>
#include <cstdint>
#include <cstring>
#include <memory>
#include <set>
#include <vector>

#include "../se_hip.h"
#include "allocate_region.hpp"
#include "octree.hpp"

namespace se {

namespace release_detail {
inline int compact21(uint64_t code, int axis) {
  int v = 0;
  for (int i = 0; i < 21; ++i) v |= (int)((code >> (3 * i + axis)) & 1ull) << i;
  return v;
}
/* v == initValue(), bit for bit, y as a float */
template <typename V> inline bool is_init(const V& v, const V& init) {
  const float a[2] = {v.x, (float)v.y}, b[2] = {init.x, (float)init.y};
  return std::memcmp(a, b, sizeof a) == 0;
}
inline bool contains(const se_hip_release_box& b, const int c[3], int d) {
  for (int k = 0; k < 3; ++k)
    if ((int64_t)c[k] < (int64_t)b.lo[k] || (int64_t)c[k] + d > (int64_t)b.lo[k] + b.side[k]) return false;
  return true;
}
}  // namespace release_detail

inline bool release_box_valid(const se_hip_release_box& b) {
  const int64_t limit = (int64_t)1 << 30;
  for (int k = 0; k < 3; ++k)
    if (b.side[k] < 1 || b.lo[k] < -limit || (int64_t)b.lo[k] + b.side[k] > limit) return false;
  return (b.what == SE_HIP_RELEASE_ALL || b.what == SE_HIP_RELEASE_UNSEEN) && b.reserved == 0;
}
inline bool release_boxes_valid(const se_hip_release_box* boxes, size_t n) {
  if (n > 4096 || (n > 0 && !boxes)) return false;
  for (size_t i = 0; i < n; ++i)
    if (!release_box_valid(boxes[i])) return false;
  return true;
}

template <typename T>
bool release_map(Octree<T>& map, const se_hip_release_box* boxes, size_t n, int64_t* counts = nullptr, int32_t* touched = nullptr) {
  typedef typename voxel_traits<T>::value_type value_type;
  if (!release_boxes_valid(boxes, n)) {
    if (counts) for (int k = 0; k < 5; ++k) counts[k] = -1;
    return false;
  }
  const value_type init = voxel_traits<T>::initValue();
  auto& nodes = map.getNodesBuffer();
  auto& blocks = map.getBlockBuffer();
  int64_t c[5] = {0, 0, 0, 0, 0};
  int box[6] = {INT32_MAX, INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, INT32_MIN};
  std::set<const Node<T>*> gone;

  /* contained by an ALL record / by any record */
  auto inside = [&](const int p[3], int d, bool& all, bool& any) {
    all = any = false;
    for (size_t i = 0; i < n; ++i)
      if (release_detail::contains(boxes[i], p, d)) { any = true; all = all || boxes[i].what == SE_HIP_RELEASE_ALL; }
  };
  /* bottom-up: is the octant released?  (its children have been decided, and the entries of a staying parent reset, when it answers) */
  struct Walk {
    static bool visit(Node<T>* o, int side, decltype(inside)& in, const value_type& init, std::set<const Node<T>*>& gone, int64_t* c, int* box) {
      const uint64_t code = o->code_ & ~0x1FFull;
      const int p[3] = {release_detail::compact21(code, 0), release_detail::compact21(code, 1), release_detail::compact21(code, 2)};
      bool all, any;
      in(p, side, all, any);
      if (o->isLeaf()) {
        auto* b = static_cast<VoxelBlock<T>*>(o);
        bool empty = true;
        for (const auto& v : b->voxel_block_) empty = empty && release_detail::is_init(v, init);
        const bool out = all || (any && empty);
        if (out) {
          ++c[1];
          if (!empty) ++c[4];
          for (int k = 0; k < 3; ++k) { box[k] = std::min(box[k], p[k]); box[3 + k] = std::max(box[3 + k], p[k] + 8); }
          gone.insert(o);
        } else ++c[0];
        return out;
      }
      bool below = true, released[8];
      for (int i = 0; i < 8; ++i) {
        released[i] = o->child_ptr_[i] ? visit(o->child_ptr_[i], side / 2, in, init, gone, c, box) : false;
        if (o->child_ptr_[i]) below = below && released[i];
      }
      bool empty = true;
      for (const auto& v : o->value_) empty = empty && release_detail::is_init(v, init);
      const bool out = (o->code_ & 0x1FFull) != 0 && (all || (any && empty)) && below;   /* (level 0: the root always stays) */
      if (out) { ++c[3]; gone.insert(o); return true; }
      ++c[2];
      for (int i = 0; i < 8; ++i)
        if (released[i]) { o->value_[i] = init; o->child_ptr_[i] = nullptr; o->children_mask_ = (unsigned char)(o->children_mask_ & ~(1 << i)); }
      return false;
    }
  };
  if (map.root()) Walk::visit(map.root(), map.size(), inside, init, gone, c, box);
  assert(c[0] + c[1] == (int64_t)blocks.size() && c[2] + c[3] == (int64_t)nodes.size());   /* (a linked snapshot: the walk met every octant) */

  auto by_key = [](const auto& p, const auto& q) { return p->code_ < q->code_; };
  std::vector<std::unique_ptr<Node<T>>> kept_nodes;
  std::vector<std::unique_ptr<VoxelBlock<T>>> kept_blocks;
  for (auto& p : nodes) if (!gone.count(p.get())) kept_nodes.push_back(std::move(p));
  for (auto& p : blocks) if (!gone.count(p.get())) kept_blocks.push_back(std::move(p));
  nodes = std::move(kept_nodes);
  blocks = std::move(kept_blocks);
  std::sort(nodes.begin(), nodes.end(), by_key);   /* (already so in a getMap() snapshot) */
  std::sort(blocks.begin(), blocks.end(), by_key);
#ifndef NDEBUG
  {
    /* the closure holds by construction: the parent of every survivor is a survivor */
    const int size = map.size();
    std::set<key_t> have;
    for (auto& p : nodes) have.insert(p->code_);
    auto parent_stays = [&](key_t key) {
      const int level = (int)(key & 0x1FFull);
      if (level == 0) return true;
      const uint64_t code = key & ~0x1FFull;
      const int d = size >> (level - 1);
      return have.count(alloc_detail::make_key(release_detail::compact21(code, 0) / d * d, release_detail::compact21(code, 1) / d * d,
                                               release_detail::compact21(code, 2) / d * d, level - 1)) == 1;
    };
    for (auto& p : nodes) assert(parent_stays(p->code_));
    for (auto& p : blocks) assert(parent_stays(p->code_));
  }
#endif
  if (counts) for (int k = 0; k < 5; ++k) counts[k] = c[k];
  if (touched) for (int k = 0; k < 6; ++k) touched[k] = c[1] ? box[k] : 0;
  return true;
}

}  // namespace se

#endif /* SE_HIP_RELEASE_MAP_HPP */
