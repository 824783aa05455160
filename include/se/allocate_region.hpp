/*
 * se::allocate_boxes on the host se::Octree snapshot that DenseSLAMSystem::getMap() materialises (include/se/octree.hpp): the executable
 * definition of the device's se_hip_allocate_boxes (include/se_hip.h) -- what DenseSLAMSystem::allocateRegion leaves in the device map is
 * what allocate_boxes makes of the snapshot taken before.
 *
 * It is the reference's Octree::allocate(key_t*, int) (se_core/include/se/octree.hpp:792-856) over the keys of every octant of a box's
 * level that the box touches inside the volume, WITHOUT the keys[0] rule of unique_multiscale (algorithms/unique.hpp:64-79: the list's
 * smallest key is kept whatever its level, so a coarse smallest key is walked down along child 0 to a leaf).  After the call every
 * requested octant and all its ancestors exist and nothing else was created; new blocks hold initValue() and are active
 * (allocate_level, octree.hpp:841), new nodes hold initValue(); what existed is untouched; list order and overlaps do not matter.
 *
 *   box.level  0 = leaf level (the 8^3 blocks); 1 .. leaf_level = the octants of that tree level (side size >> level), created as nodes
 *              without children below them (leaf_level names the blocks again)
 *   invalid    a coordinate of lo or hi outside [-2^30, 2^30]; level outside 0 .. leaf_level; reserved != 0: skipped whole, counted
 *   counts     (optional, int64[4]) blocks created, nodes created (ancestors included), requested (box, octant) pairs after clipping,
 *              invalid boxes
 *   new_keys   (optional) the keys (Morton code of the corner | level) of the octants created because a box requested them.  A requested
 *              octant that came into being earlier in the call as the ancestor of a finer request is not listed (that request's key implies
 *              it), and which of the two comes first is unspecified on the device.  What holds in any order: every key names a requested
 *              octant that did not exist before, none appears twice, and the ancestor closure of the keys together with the map before is
 *              the map after.
 * The snapshot's buffers are in key order afterwards, as getMap() delivers them, and the tree is linked.
 */
#ifndef SE_HIP_ALLOCATE_REGION_HPP
#define SE_HIP_ALLOCATE_REGION_HPP

#include <algorithm>
#include <cstdint>
#include <memory>
#include <set>
#include <vector>

#include "../se_hip.h"
#include "octree.hpp"

namespace se {

namespace alloc_detail {
inline uint64_t spread21(uint64_t v) {
  uint64_t r = 0;
  for (int i = 0; i < 21; ++i) r |= ((v >> i) & 1ull) << (3 * i);
  return r;
}
/* the key of the octant with voxel corner (x, y, z) at `level` (octant_ops.hpp:49-53) */
inline key_t make_key(int x, int y, int z, int level) { return spread21((uint64_t)x) | (spread21((uint64_t)y) << 1) | (spread21((uint64_t)z) << 2) | (key_t)level; }
}  // namespace alloc_detail

/* is the box one the call skips whole? (reads the record only) */
inline bool alloc_box_valid(const se_hip_alloc_box& b, int leaf_level) {
  const int limit = 1 << 30;
  for (int k = 0; k < 3; ++k)
    if (b.lo[k] < -limit || b.lo[k] > limit || b.hi[k] < -limit || b.hi[k] > limit) return false;
  return b.reserved == 0u && b.level >= 0 && b.level <= leaf_level;
}

template <typename T>
void allocate_boxes(Octree<T>& map, const se_hip_alloc_box* boxes, size_t n, int64_t* counts = nullptr, std::vector<key_t>* new_keys = nullptr) {
  const int size = map.size();
  int max_level = 0;
  for (int s = size; s > 1; s >>= 1) ++max_level;
  const int leaf_level = max_level - 3;
  int64_t c[4] = {0, 0, 0, 0};
  if (new_keys) new_keys->clear();
  std::set<key_t> have;
  for (auto& p : map.getNodesBuffer()) have.insert(p->code_);
  for (auto& p : map.getBlockBuffer()) have.insert(p->code_);
  if (!have.count(0)) { map.add_node(0, (unsigned)size); have.insert(0); }   /* Octree::init creates the root */
  /* creates the octant with corner (x, y, z) at `level` if it is absent; true if it did */
  auto create = [&](int x, int y, int z, int level) {
    const key_t key = alloc_detail::make_key(x, y, z, level);
    if (!have.insert(key).second) return false;
    if (level == leaf_level) { const int corner[3] = {x, y, z}; map.add_block(key, corner, true); ++c[0]; }
    else { map.add_node(key, (unsigned)(size >> level)); ++c[1]; }
    return true;
  };
  for (size_t i = 0; i < n; ++i) {
    const se_hip_alloc_box& b = boxes[i];
    if (!alloc_box_valid(b, leaf_level)) { ++c[3]; continue; }
    const int level = b.level == 0 ? leaf_level : b.level;
    const int side = size >> level;
    int lo[3], hi[3];
    bool empty = false;
    for (int k = 0; k < 3; ++k) {
      const int l = std::max(b.lo[k], 0), h = std::min(b.hi[k], size);
      empty = empty || l >= h;
      lo[k] = l / side; hi[k] = empty ? lo[k] : (h - 1) / side + 1;   /* octants of the level the clipped box touches */
    }
    if (empty) continue;
    for (int z = lo[2]; z < hi[2]; ++z)
      for (int y = lo[1]; y < hi[1]; ++y)
        for (int x = lo[0]; x < hi[0]; ++x) {
          ++c[2];
          if (!create(x * side, y * side, z * side, level)) continue;
          if (new_keys) new_keys->push_back(alloc_detail::make_key(x * side, y * side, z * side, level));
          for (int l = level - 1; l >= 1; --l) {   /* the ancestors; the first that exists has all of its own */
            const int s = size >> l;
            if (!create(x * side / s * s, y * side / s * s, z * side / s * s, l)) break;
          }
        }
  }
  auto by_key = [](const auto& p, const auto& q) { return p->code_ < q->code_; };
  std::sort(map.getNodesBuffer().begin(), map.getNodesBuffer().end(), by_key);
  std::sort(map.getBlockBuffer().begin(), map.getBlockBuffer().end(), by_key);
  map.finalize();
  if (counts) for (int k = 0; k < 4; ++k) counts[k] = c[k];
}

}  // namespace se

#endif /* SE_HIP_ALLOCATE_REGION_HPP */
