/*
 * se::geometry collision queries on the host se::Octree snapshot that DenseSLAMSystem::getMap() materialises (include/se/octree.hpp):
 * the reference's map read algorithm collides_with (se_core/include/se/geometry/octree_collision.hpp:74-167) and its overlap test
 * (aabb_collision.hpp), restated for this mirror without Eigen.  Box corners and extents are any 3-vector type with operator()(int)
 * (Eigen::Vector3i in the reference; se::geometry::int3 below works too).
 *
 * This is the literal sequential traversal -- an explicit stack, children pushed in order 0..7 -- with the reference's quirks kept:
 *   - the overlap test is inclusive on integer midpoints, for octants and for voxels (a box of side 2 touches 3 voxels per axis);
 *   - an absent overlapping child is judged by its parent's value_[0];
 *   - a visited leaf's status replaces the running status;
 *   - the root is always visited and not itself tested; a node without children adds nothing.
 * It is the independent model of the device's SE_HIP_COLLIDE_REFERENCE mode (include/se_hip.h, which also defines SE_HIP_COLLIDE_STRICT).
 * Integer sums are taken in 64 bits, so a box as large as the C ABI accepts cannot overflow the test.
 */
#ifndef SE_HIP_OCTREE_COLLISION_HPP
#define SE_HIP_OCTREE_COLLISION_HPP

#include <cstdint>
#include <vector>

#include "octree.hpp"

namespace se {
namespace geometry {

/* in the order of the reference's enum: occupied, unseen, empty (the C ABI's status codes 0, 1, 2) */
enum class collision_status { occupied, unseen, empty };

/* the reference's severity state machine: occupied beats unseen beats empty */
inline collision_status update_status(const collision_status previous, const collision_status next) {
  if (previous == collision_status::occupied) return previous;
  if (previous == collision_status::unseen) return next == collision_status::occupied ? next : previous;
  return next;
}

/* one axis of the inclusive overlap test: the segments [a, a + a_edge] and [b, b + b_edge] compared by their integer midpoints */
inline int axis_overlap(const int a, const int a_edge, const int b, const int b_edge) {
  const int64_t mid_a = (int64_t)a + a_edge / 2, mid_b = (int64_t)b + b_edge / 2;
  const int64_t d = mid_b > mid_a ? mid_b - mid_a : mid_a - mid_b;
  return d > ((int64_t)a_edge + b_edge) / 2 ? 0 : 1;
}

template <typename Vec3i, typename Vec3j>
inline int aabb_aabb_collision(const Vec3i& a, const Vec3i& a_edge, const Vec3j& b, const Vec3j& b_edge) {
  return axis_overlap(a(0), a_edge(0), b(0), b_edge(0)) && axis_overlap(a(1), a_edge(1), b(1), b_edge(1)) &&
         axis_overlap(a(2), a_edge(2), b(2), b_edge(2));
}

/* a minimal integer 3-vector for callers without Eigen */
struct int3 {
  int v[3];
  int operator()(int i) const { return v[i]; }
  int& operator()(int i) { return v[i]; }
};

/* The classification the C ABI's se_hip_collide_test describes: unseen where the value equals initValue(), else occupied where
 * x > threshold (occupied_above) or x < threshold, else empty.  (The reference's own test functor uses the same unseen rule.) */
template <typename T>
struct voxel_test {
  float threshold;
  bool occupied_above;
  template <typename V>
  collision_status operator()(const V& v) const {
    const auto init = voxel_traits<T>::initValue();
    if (v.x == init.x && v.y == init.y) return collision_status::unseen;
    return (occupied_above ? v.x > threshold : v.x < threshold) ? collision_status::occupied : collision_status::empty;
  }
};

/* every voxel of `block` that passes the overlap test with the box, folded from empty */
template <typename T, typename Vec3i, typename TestF>
collision_status collides_with(const VoxelBlock<T>* block, const Vec3i& bbox, const Vec3i& side, TestF test) {
  collision_status status = collision_status::empty;
  const int* c = block->coordinates();
  const int n = (int)VoxelBlock<T>::side;
  const int3 one = {{1, 1, 1}};
  for (int z = c[2]; z < c[2] + n; ++z)
    for (int y = c[1]; y < c[1] + n; ++y)
      for (int x = c[0]; x < c[0] + n; ++x) {
        const int3 v = {{x, y, z}};
        if (!aabb_aabb_collision(bbox, side, v, one)) continue;
        status = update_status(status, test(block->data(x, y, z)));
      }
  return status;
}

/* the box [bbox, bbox + side] (in the reference's inclusive sense) against the whole map */
template <typename T, typename Vec3i, typename TestF>
collision_status collides_with(const Octree<T>& map, const Vec3i& bbox, const Vec3i& side, TestF test) {
  struct entry { Node<T>* node; int x, y, z, side; };
  Node<T>* root = map.root();
  if (!root) return collision_status::unseen;
  std::vector<entry> stack;
  stack.push_back({root, 0, 0, 0, map.size()});
  entry cur = stack.back();
  collision_status status = collision_status::empty;
  /* as in the reference, the root stays at the bottom of the stack: the loop ends when it would be taken a second time */
  while (!stack.empty()) {
    Node<T>* node = cur.node;
    if (node->isLeaf()) status = collides_with(static_cast<const VoxelBlock<T>*>(node), bbox, side, test);
    if (node->children_mask_ != 0) {
      const int half = cur.side / 2;
      for (int i = 0; i < 8; ++i) {
        const int3 corner = {{cur.x + ((i & 1) ? half : 0), cur.y + ((i & 2) ? half : 0), cur.z + ((i & 4) ? half : 0)}};
        const int3 edge = {{half, half, half}};
        if (!aabb_aabb_collision(bbox, side, corner, edge)) continue;
        Node<T>* child = node->child(i);
        if (child) stack.push_back({child, corner(0), corner(1), corner(2), half});
        else status = update_status(status, test(node->value_[0]));
      }
    }
    cur = stack.back();
    stack.pop_back();
  }
  return status;
}

}  // namespace geometry
}  // namespace se

#endif /* SE_HIP_OCTREE_COLLISION_HPP */
