/*
 * se::merge_map_rigid on two host se::Octree snapshots that DenseSLAMSystem::getMap() materialises (include/se/octree.hpp): the executable
 * definition of the device's se_hip_merge_map_rigid (include/se_hip.h) -- what DenseSLAMSystem::mergeMapRigid leaves in the device map is
 * what merge_map_rigid makes of the two snapshots taken before.  The reference has no counterpart: it holds one map.
 *
 * pull = src_from_dst, row-major 3 x 4, in voxels: R = its first three columns, t = the fourth.  Nothing is inverted here.
 *
 *   convention a voxel with integer coordinates v holds the field at position v, in voxels (Octree::interp's convention: the cell's lower
 *              corner is floor(q)); there is no half-voxel offset
 *   position   for a destination voxel v: q_k = ((R_k0 * vx + R_k1 * vy) + R_k2 * vz) + t_k, binary32 in that order, no contraction (build
 *              with -ffp-contract=off); l = floor(q), f = q - floorf(q)
 *   validity   rigid_sample: the sample is valid iff 0 <= l_k and l_k + 1 <= src size - 1 on every axis and none of the eight corner
 *              voxels l + {0,1}^3 is unseen.  Corners are read with get_fine (initValue() where the source has no block); "unseen":
 *              x == initValue().x && y == initValue().y, y compared as float.  A cell with any unseen corner contributes nothing: no
 *              extrapolation, no empty() substitution
 *   value      b.x = the blend of the corner x values p[i + 2j + 4k] in Octree::interp's term order (octree.hpp:553-562),
 *                ((p0 (1-fx) + p1 fx) (1-fy) + (p2 (1-fx) + p3 fx) fy) (1-fz) + ((p4 (1-fx) + p5 fx) (1-fy) + (p6 (1-fx) + p7 fx) fy) fz;
 *              SDF: b.y = the minimum of the eight corner weights; OFusion: b.y = the maximum of the eight corner times.
 *              The sample is observed iff it is valid and b itself is not unseen
 *   values     every destination voxel with an observed sample becomes se::merge_value(a, b, mode, max_weight) (merge_map.hpp), exactly
 *              as it stands; every other voxel keeps its bits
 *   blocks     an absent destination block is created iff at least one of its 512 voxels has an observed sample, with all missing ancestors
 *              and initValue() (Octree::allocate, allocate_region.hpp: without the keys[0] rule); no other block is created.  Every
 *              destination block that receives at least one observed sample is active afterwards, as insertion leaves a new block
 *   nodes      source node values never take part: coarse values cannot be resampled.  Destination node values are untouched; ancestors
 *              created on the way hold initValue()
 *   arguments  merge_rigid_valid: both trees distinct, dim / size (a binary32 division) bit-equal, every entry of pull finite,
 *              |t_k| <= 2^20, max |R^T R - I| <= 1e-3 and det R > 0 (both in double: rigid, no scale, no mirror), a known mode, max_weight
 *              an integer in [1, 255]; anything else leaves both maps untouched (counts all -1).  The sizes may differ
 *   counts     (optional, int64[10]) blocks that existed and received an observed sample, blocks created, voxels with an observed sample,
 *              of those the voxels whose destination value was observed before, lo[3] and hi[3] of the half-open destination voxel box over
 *              the blocks that received samples (all zero if none)
 * Non-finite source values: the library never produces them; the result for them is unspecified.
 * The destination's buffers are in key order afterwards, as getMap() delivers them, and the tree is linked.  The source is only read.
 */
#ifndef SE_HIP_MERGE_RIGID_HPP
#define SE_HIP_MERGE_RIGID_HPP

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <type_traits>
#include <vector>

#include "allocate_region.hpp"
#include "merge_map.hpp"
#include "octree.hpp"

namespace se {

namespace rigid_detail {
template <typename V> inline bool unseen(const V& v, const V& init) { return v.x == init.x && (float)v.y == (float)init.y; }
}  // namespace rigid_detail

inline bool rigid_pull_valid(const float pull[12]) {
  if (!pull) return false;
  for (int k = 0; k < 12; ++k) if (!std::isfinite(pull[k])) return false;
  double R[3][3];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) R[r][c] = (double)pull[4 * r + c];
    if (std::fabs((double)pull[4 * r + 3]) > 1048576.0) return false;
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double g = (R[0][i] * R[0][j] + R[1][i] * R[1][j]) + R[2][i] * R[2][j];
      if (std::fabs(g - (i == j ? 1.0 : 0.0)) > 1e-3) return false;
    }
  const double det = R[0][0] * (R[1][1] * R[2][2] - R[1][2] * R[2][1]) - R[0][1] * (R[1][0] * R[2][2] - R[1][2] * R[2][0]) +
                     R[0][2] * (R[1][0] * R[2][1] - R[1][1] * R[2][0]);
  return det > 0.0;
}

template <typename T>
bool merge_rigid_valid(const Octree<T>& dst, const Octree<T>& src, const float pull[12], const merge_rule& rule) {
  if (&dst == &src || dst.size() <= 0 || src.size() <= 0) return false;
  const float va = dst.dim() / (float)dst.size(), vb = src.dim() / (float)src.size();
  if (std::memcmp(&va, &vb, sizeof va) != 0) return false;
  if (!rigid_pull_valid(pull)) return false;
  if (rule.mode != MERGE_FUSE && rule.mode != MERGE_REPLACE && rule.mode != MERGE_FILL) return false;
  return rule.max_weight >= 1.f && rule.max_weight <= 255.f && rule.max_weight == (float)(int)rule.max_weight;
}

/* the source field at position q (voxels): false if the sample is not valid, else *b = the sample */
template <typename T>
bool rigid_sample(const Octree<T>& src, const float q[3], typename voxel_traits<T>::value_type* b) {
  typedef typename voxel_traits<T>::value_type value_type;
  const bool sdf = std::is_same<T, SDF>::value;
  const value_type init = voxel_traits<T>::initValue();
  float fl[3], f[3];
  int l[3];
  for (int k = 0; k < 3; ++k) {
    fl[k] = floorf(q[k]);
    if (!(fl[k] >= 0.f && fl[k] <= (float)(src.size() - 2))) return false;
    l[k] = (int)fl[k];
    f[k] = q[k] - fl[k];
  }
  float p[8];
  float y = 0.f;
  for (int c = 0; c < 8; ++c) {
    const value_type v = src.get_fine(l[0] + (c & 1), l[1] + ((c >> 1) & 1), l[2] + (c >> 2));
    if (rigid_detail::unseen(v, init)) return false;
    p[c] = v.x;
    const float vy = (float)v.y;
    y = c == 0 ? vy : (sdf ? fminf(y, vy) : fmaxf(y, vy));
  }
  b->x = (((p[0] * (1 - f[0]) + p[1] * f[0]) * (1 - f[1]) + (p[2] * (1 - f[0]) + p[3] * f[0]) * f[1]) * (1 - f[2]) +
          ((p[4] * (1 - f[0]) + p[5] * f[0]) * (1 - f[1]) + (p[6] * (1 - f[0]) + p[7] * f[0]) * f[1]) * f[2]);
  b->y = y;
  return true;
}

template <typename T>
void merge_map_rigid(Octree<T>& dst, Octree<T>& src, const float pull[12], const merge_rule& rule = merge_rule(), int64_t* counts = nullptr) {
  typedef typename voxel_traits<T>::value_type value_type;
  if (!merge_rigid_valid(dst, src, pull, rule)) {
    if (counts) for (int k = 0; k < 10; ++k) counts[k] = -1;
    return;
  }
  const int size = dst.size();
  int max_level = 0;
  for (int v = size; v > 1; v >>= 1) ++max_level;
  const int leaf_level = max_level - 3;
  const value_type init = voxel_traits<T>::initValue();
  auto& nodes = dst.getNodesBuffer();
  auto& blocks = dst.getBlockBuffer();
  std::map<key_t, Node<T>*> have_n;
  std::map<key_t, VoxelBlock<T>*> have_b;
  for (auto& n : nodes) have_n[n->code_] = n.get();
  for (auto& b : blocks) have_b[b->code_] = b.get();
  if (!have_n.count(0)) have_n[0] = dst.add_node(0, (unsigned)size);   /* (a snapshot always holds the root) */
  int64_t c[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  bool any = false;
  std::vector<value_type> sample(512);
  std::vector<char> seen(512);
  for (int bz = 0; bz < size; bz += 8)
    for (int by = 0; by < size; by += 8)
      for (int bx = 0; bx < size; bx += 8) {
        int n_seen = 0;
        for (int j = 0; j < 512; ++j) {
          const float vx = (float)(bx + (j & 7)), vy = (float)(by + ((j >> 3) & 7)), vz = (float)(bz + (j >> 6));
          float q[3];
          for (int k = 0; k < 3; ++k) q[k] = ((pull[4 * k] * vx + pull[4 * k + 1] * vy) + pull[4 * k + 2] * vz) + pull[4 * k + 3];
          seen[j] = rigid_sample<T>(src, q, &sample[j]) && !rigid_detail::unseen(sample[j], init);
          n_seen += seen[j];
        }
        if (!n_seen) continue;
        const int corner[3] = {bx, by, bz};
        const key_t key = alloc_detail::make_key(bx, by, bz, leaf_level);
        VoxelBlock<T>* t = nullptr;
        auto it = have_b.find(key);
        if (it != have_b.end()) { t = it->second; ++c[0]; }
        else {
          t = dst.add_block(key, corner, true);
          have_b[key] = t;
          ++c[1];
          for (int l = leaf_level - 1; l >= 1; --l) {   /* every missing ancestor, with initValue(); the first that exists has all of its own */
            const int d = size >> l;
            const key_t up = alloc_detail::make_key(bx / d * d, by / d * d, bz / d * d, l);
            if (have_n.count(up)) break;
            have_n[up] = dst.add_node(up, (unsigned)d);
          }
        }
        for (int j = 0; j < 512; ++j) {
          if (!seen[j]) continue;
          ++c[2];
          if (!rigid_detail::unseen(t->voxel_block_[j], init)) ++c[3];
          t->voxel_block_[j] = merge_value<T>(t->voxel_block_[j], sample[j], rule.mode, rule.max_weight);
        }
        t->active_ = true;
        for (int k = 0; k < 3; ++k) {
          c[4 + k] = any ? std::min<int64_t>(c[4 + k], corner[k]) : corner[k];
          c[7 + k] = any ? std::max<int64_t>(c[7 + k], corner[k] + 8) : corner[k] + 8;
        }
        any = true;
      }
  auto by_key = [](const auto& p, const auto& q) { return p->code_ < q->code_; };
  std::sort(nodes.begin(), nodes.end(), by_key);
  std::sort(blocks.begin(), blocks.end(), by_key);
  dst.finalize();
  if (counts) for (int k = 0; k < 10; ++k) counts[k] = c[k];
}

}  // namespace se

#endif /* SE_HIP_MERGE_RIGID_HPP */
