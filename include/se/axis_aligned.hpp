/*
 * se::functor::axis_aligned_map on the host se::Octree snapshot that DenseSLAMSystem::getMap() materialises (include/se/octree.hpp): the
 * reference's map write algorithm (se_core/include/se/functors/axis_aligned_functor.hpp, handlers of functors/data_handler.hpp) restated
 * for this mirror, so that user code written against the reference
 *
 *     se::functor::axis_aligned_map(map, [](auto& handler, const Eigen::Vector3i& v) { handler.set(...); }, min, max);
 *
 * compiles against a snapshot -- and se::apply_edits, the executable definition of the device's se_hip_edit_boxes (include/se_hip.h):
 * what DenseSLAMSystem::editMap leaves in the device map is what apply_edits makes of the snapshot taken before.
 *
 * axis_aligned_map(map, f, min, max) visits
 *   - every voxel v of every allocated block with min <= v < max per axis (update_block: the block's range clipped to the box), x fastest;
 *   - every value_[i] of every node, at the position the reference computes: unpack_morton(code_) WITH the level bits still in the code,
 *     advanced cumulatively by dir(i) * side / 2 over i, tested inclusively (min <= v <= max) -- with h = side / 2 the eight positions are
 *     c0 + (0,0,0), (h,0,0), (h,h,0), (2h,2h,0), (2h,2h,h), (3h,2h,2h), (3h,3h,3h), (4h,4h,4h).
 * Blocks first, then nodes, each in buffer order (the reference runs them under OpenMP: its order is unspecified).  A box whose max lies
 * below a block's corner selects nothing here; the reference's unsigned loop counters make that case undefined there.
 */
#ifndef SE_HIP_AXIS_ALIGNED_HPP
#define SE_HIP_AXIS_ALIGNED_HPP

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "../se_hip.h"
#include "eigen_pods.h"
#include "octree.hpp"
#include "octree_collision.hpp"

namespace se {

/* functors/data_handler.hpp: what the update function is handed -- one voxel of a block, or one value_[i] of a node */
template <typename T> class VoxelBlockHandler {
 public:
  typedef typename voxel_traits<T>::value_type value_type;
  VoxelBlockHandler(VoxelBlock<T>* block, const Eigen::Vector3i& voxel) : block_(block), voxel_(voxel) {}
  value_type get() { return block_->voxel_block_[index()]; }
  void set(const value_type& v) { block_->voxel_block_[index()] = v; }

 private:
  int index() const {
    const int* c = block_->coordinates();
    return (voxel_(0) - c[0]) + 8 * (voxel_(1) - c[1]) + 64 * (voxel_(2) - c[2]);
  }
  VoxelBlock<T>* block_;
  Eigen::Vector3i voxel_;
};

template <typename T> class NodeHandler {
 public:
  typedef typename voxel_traits<T>::value_type value_type;
  NodeHandler(Node<T>* node, int i) : node_(node), i_(i) {}
  value_type get() { return node_->value_[i_]; }
  void set(const value_type& v) { node_->value_[i_] = v; }

 private:
  Node<T>* node_;
  int i_;
};

namespace functor {

/* axis `axis` of unpack_morton(code): bits 3i + axis of the whole key, the level in its low bits included */
inline int unpack_axis(key_t code, int axis) {
  int v = 0;
  for (int i = 0; i < 21; ++i) v |= (int)((code >> (3 * i + axis)) & 1ull) << i;
  return v;
}

/* the eight positions update_node tests for `node`, in order */
template <typename T> inline void node_positions(const Node<T>& node, int out[8][3]) {
  int v[3] = {unpack_axis(node.code_, 0), unpack_axis(node.code_, 1), unpack_axis(node.code_, 2)};
  const int h = (int)(node.side_ / 2);
  for (int i = 0; i < 8; ++i) {
    for (int k = 0; k < 3; ++k) { v[k] += ((i >> k) & 1) * h; out[i][k] = v[k]; }
  }
}

template <typename T, typename UpdateF>
void axis_aligned_map(Octree<T>& map, UpdateF f, const Eigen::Vector3i& min, const Eigen::Vector3i& max) {
  for (auto& b : map.getBlockBuffer()) {
    const int* c = b->coordinates();
    int first[3], last[3];
    for (int k = 0; k < 3; ++k) { first[k] = c[k] > min(k) ? c[k] : min(k); last[k] = c[k] + 8 < max(k) ? c[k] + 8 : max(k); }
    for (int z = first[2]; z < last[2]; ++z)
      for (int y = first[1]; y < last[1]; ++y)
        for (int x = first[0]; x < last[0]; ++x) {
          const Eigen::Vector3i vox(x, y, z);
          VoxelBlockHandler<T> handler(b.get(), vox);
          f(handler, vox);
        }
  }
  for (auto& n : map.getNodesBuffer()) {
    int pos[8][3];
    node_positions(*n, pos);
    for (int i = 0; i < 8; ++i) {
      bool in = true;
      for (int k = 0; k < 3; ++k) in = in && pos[i][k] >= min(k) && pos[i][k] <= max(k);
      if (!in) continue;
      const Eigen::Vector3i vox(pos[i][0], pos[i][1], pos[i][2]);
      NodeHandler<T> handler(n.get(), i);
      f(handler, vox);
    }
  }
}

template <typename T, typename UpdateF>
void axis_aligned_map(Octree<T>& map, UpdateF f) {
  axis_aligned_map(map, f, Eigen::Vector3i(0, 0, 0), Eigen::Vector3i(map.size(), map.size(), map.size()));
}

}  // namespace functor

/* ---- the edit list of se_hip_edit_boxes (definitions in include/se_hip.h) */

/* is `test` usable for a class predicate? */
inline bool edit_test_ok(const se_hip_collide_test* test) {
  return test && std::isfinite(test->threshold) && (test->occupied_above == 0 || test->occupied_above == 1);
}

/* the "invalid edit" rules for field type T */
template <typename T> inline bool edit_valid(const se_hip_edit& e, const se_hip_collide_test* test) {
  const int32_t limit = 1 << 30;
  for (int k = 0; k < 3; ++k)
    if (e.lo[k] < -limit || e.lo[k] > limit || e.hi[k] < -limit || e.hi[k] > limit) return false;
  if (e.flags & ~(SE_HIP_EDIT_SET_X | SE_HIP_EDIT_SET_Y | SE_HIP_EDIT_BLOCKS | SE_HIP_EDIT_NODES)) return false;
  if (e.only < 1u || e.only > 7u) return false;
  if (e.only != 7u && !edit_test_ok(test)) return false;
  if ((e.flags & SE_HIP_EDIT_SET_X) && !std::isfinite(e.x)) return false;
  if (e.flags & SE_HIP_EDIT_SET_Y) {
    if (!std::isfinite(e.y)) return false;
    if (std::is_same<T, SDF>::value && !(e.y >= 0.f && e.y <= 255.f && e.y == std::floor(e.y))) return false;
  }
  return true;
}

/* Applies the n edits to `map` as if one after another in list order.  Written value by value -- each voxel and each node value walks
 * the list -- which is how the device evaluates it; tests/cpp/edit_kats.cpp checks it against the edit-by-edit loop over axis_aligned_map.
 * mode: SE_HIP_EDIT_STRICT or SE_HIP_EDIT_REFERENCE (anything else: nothing is done, false).  counts (optional): as se_hip_edit_boxes. */
template <typename T>
bool apply_edits(Octree<T>& map, const se_hip_edit* edits, size_t n, const se_hip_collide_test* test, int32_t mode, int64_t* counts = nullptr) {
  typedef typename voxel_traits<T>::value_type value_type;
  if (mode != SE_HIP_EDIT_STRICT && mode != SE_HIP_EDIT_REFERENCE) return false;
  int64_t cnt[4] = {0, 0, 0, 0};
  std::vector<unsigned char> valid(n);
  for (size_t i = 0; i < n; ++i) { valid[i] = edit_valid<T>(edits[i], test) ? 1 : 0; cnt[3] += valid[i] ? 0 : 1; }
  const geometry::voxel_test<T> classify = {edit_test_ok(test) ? test->threshold : 0.f, edit_test_ok(test) && test->occupied_above != 0};
  /* one value under one edit whose box test it has passed */
  auto visit = [&](value_type& v, const se_hip_edit& e) -> bool {
    if (e.only != 7u && !((e.only >> (unsigned)classify(v)) & 1u)) return false;
    if (e.flags & SE_HIP_EDIT_SET_X) v.x = e.x;
    if (e.flags & SE_HIP_EDIT_SET_Y) v.y = e.y;
    return true;
  };
  for (auto& b : map.getBlockBuffer()) {
    const int* c = b->coordinates();
    int64_t here = 0;
    for (int v = 0; v < 512; ++v) {
      const int p[3] = {c[0] + (v & 7), c[1] + ((v >> 3) & 7), c[2] + (v >> 6)};
      for (size_t i = 0; i < n; ++i) {
        const se_hip_edit& e = edits[i];
        if (!valid[i] || !(e.flags & SE_HIP_EDIT_BLOCKS)) continue;
        if (p[0] < e.lo[0] || p[0] >= e.hi[0] || p[1] < e.lo[1] || p[1] >= e.hi[1] || p[2] < e.lo[2] || p[2] >= e.hi[2]) continue;
        if (visit(b->voxel_block_[v], e)) ++here;
      }
    }
    cnt[0] += here;
    cnt[2] += here ? 1 : 0;
  }
  for (auto& nd : map.getNodesBuffer()) {
    int pos[8][3];
    functor::node_positions(*nd, pos);
    /* the node's true corner: the code without its level bits (the corner is a multiple of side >= 16: the low 12 bits are the level's alone) */
    const key_t morton = nd->code_ & ~(key_t)0xFFF;
    const int corner[3] = {functor::unpack_axis(morton, 0), functor::unpack_axis(morton, 1), functor::unpack_axis(morton, 2)};
    const int h = (int)(nd->side_ / 2);
    for (int j = 0; j < 8; ++j) {
      for (size_t i = 0; i < n; ++i) {
        const se_hip_edit& e = edits[i];
        if (!valid[i] || !(e.flags & SE_HIP_EDIT_NODES)) continue;
        bool in = true;
        for (int k = 0; k < 3; ++k) {
          if (mode == SE_HIP_EDIT_REFERENCE) in = in && e.lo[k] <= pos[j][k] && pos[j][k] <= e.hi[k];
          else { const int q = corner[k] + ((j >> k) & 1) * h; in = in && e.lo[k] <= q && q + h <= e.hi[k]; }
        }
        if (in && visit(nd->value_[j], e)) ++cnt[1];
      }
    }
  }
  if (counts) for (int k = 0; k < 4; ++k) counts[k] = cnt[k];
  return true;
}

}  // namespace se

#endif /* SE_HIP_AXIS_ALIGNED_HPP */
