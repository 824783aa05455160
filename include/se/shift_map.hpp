/*
 * se::shift_map on the host se::Octree snapshot that DenseSLAMSystem::getMap() materialises (include/se/octree.hpp): the executable
 * definition of the device's se_hip_shift_map (include/se_hip.h) -- what DenseSLAMSystem::shiftMap leaves in the device map is what
 * shift_map makes of the snapshot taken before.  The reference has no counterpart: its volume is a fixed cube and nothing in it is freed.
 *
 * The map content is translated by a whole number of blocks: content at voxel c before the call is at c + s after it.  What leaves the
 * cube is forgotten, the vacated side is unseen.
 *
 *   arguments  every component of s a multiple of 8 (the block side) within [-2^30, 2^30]; anything else leaves the map untouched
 *              (shift_valid; counts are then all -1).  s = 0 is valid and changes nothing.
 *   blocks     the block with corner c survives iff c + s lies in [0, size - 8] on every axis.  It keeps all 512 values and active_.
 *   nodes      the internal node with side d and corner c survives iff s = 0 (mod d) on every axis and c + s lies in [0, size - d]; the
 *              root follows the same rule, so it survives only for s = 0.  A survivor keeps value_[8].  A node the shift is not aligned
 *              to is dropped: its children would no longer be its children.
 *   closure    every missing ancestor of a survivor is created with initValue(), as Octree::allocate creates it (allocate_region.hpp:
 *              without the keys[0] rule); the root always exists afterwards.  Nothing else exists; surviving childless nodes stay.
 *   counts     (optional, int64[4]) blocks kept, blocks dropped, nodes kept, nodes dropped -- the root among the nodes: kept for s = 0,
 *              dropped otherwise (the root that exists afterwards is then a new one).
 * The snapshot's buffers are in key order afterwards, as getMap() delivers them, and the tree is linked.
 */
#ifndef SE_HIP_SHIFT_MAP_HPP
#define SE_HIP_SHIFT_MAP_HPP

#include <algorithm>
#include <cstdint>
#include <memory>
#include <set>
#include <vector>

#include "allocate_region.hpp"
#include "octree.hpp"

namespace se {

namespace shift_detail {
inline int compact21(uint64_t code, int axis) {
  int v = 0;
  for (int i = 0; i < 21; ++i) v |= (int)((code >> (3 * i + axis)) & 1ull) << i;
  return v;
}
}  // namespace shift_detail

inline bool shift_valid(const int s[3]) {
  const int limit = 1 << 30;
  for (int k = 0; k < 3; ++k)
    if (s[k] < -limit || s[k] > limit || (s[k] & 7) != 0) return false;
  return true;
}

template <typename T>
void shift_map(Octree<T>& map, const int s[3], int64_t* counts = nullptr) {
  if (!shift_valid(s)) {
    if (counts) for (int k = 0; k < 4; ++k) counts[k] = -1;
    return;
  }
  const int size = map.size();
  int max_level = 0;
  for (int v = size; v > 1; v >>= 1) ++max_level;
  const int leaf_level = max_level - 3;
  auto& nodes = map.getNodesBuffer();
  auto& blocks = map.getBlockBuffer();
  int64_t c[4] = {0, 0, 0, 0};
  auto by_key = [](const auto& p, const auto& q) { return p->code_ < q->code_; };
  if (s[0] == 0 && s[1] == 0 && s[2] == 0) {
    std::sort(nodes.begin(), nodes.end(), by_key);   /* (already so in a getMap() snapshot) */
    std::sort(blocks.begin(), blocks.end(), by_key);
    if (counts) { counts[0] = (int64_t)blocks.size(); counts[1] = 0; counts[2] = (int64_t)nodes.size(); counts[3] = 0; }
    return;
  }
  /* does the octant with side d and corner p survive?  q = its corner afterwards */
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
  std::vector<std::unique_ptr<Node<T>>> kept_nodes;
  std::vector<std::unique_ptr<VoxelBlock<T>>> kept_blocks;
  std::set<key_t> have;
  for (auto& n : nodes) {
    const int level = (int)(n->code_ & 0x1FFull);
    const key_t code = n->code_ & ~0x1FFull;
    const int p[3] = {shift_detail::compact21(code, 0), shift_detail::compact21(code, 1), shift_detail::compact21(code, 2)};
    int q[3];
    if (!moved(p, size >> level, q)) { ++c[3]; continue; }   /* (the root among them: a nonzero s that `size` divides moves it out of the cube) */
    n->code_ = alloc_detail::make_key(q[0], q[1], q[2], level);
    n->children_mask_ = 0;
    for (auto& ch : n->child_ptr_) ch = nullptr;
    have.insert(n->code_);
    kept_nodes.push_back(std::move(n));
    ++c[2];
  }
  for (auto& b : blocks) {
    int q[3];
    if (!moved(b->coordinates_, 8, q)) { ++c[1]; continue; }
    b->code_ = alloc_detail::make_key(q[0], q[1], q[2], leaf_level);
    for (int k = 0; k < 3; ++k) b->coordinates_[k] = q[k];
    have.insert(b->code_);
    kept_blocks.push_back(std::move(b));
    ++c[0];
  }
  nodes = std::move(kept_nodes);
  blocks = std::move(kept_blocks);
  /* the closure: the root, and every missing ancestor of a survivor, with initValue() */
  map.add_node(0, (unsigned)size);
  have.insert(0);
  std::vector<key_t> survivors(have.begin(), have.end());
  for (key_t key : survivors) {
    const int level = (int)(key & 0x1FFull);
    const key_t code = key & ~0x1FFull;
    const int p[3] = {shift_detail::compact21(code, 0), shift_detail::compact21(code, 1), shift_detail::compact21(code, 2)};
    for (int l = level - 1; l >= 1; --l) {
      const int d = size >> l;
      const key_t up = alloc_detail::make_key(p[0] / d * d, p[1] / d * d, p[2] / d * d, l);
      if (!have.insert(up).second) break;   /* the first that exists has all of its own */
      map.add_node(up, (unsigned)d);
    }
  }
  std::sort(nodes.begin(), nodes.end(), by_key);
  std::sort(blocks.begin(), blocks.end(), by_key);
  map.finalize();
  if (counts) for (int k = 0; k < 4; ++k) counts[k] = c[k];
}

}  // namespace se

#endif /* SE_HIP_SHIFT_MAP_HPP */
