/*
 * Column projections -- per cell of a 2D footprint and per interval along the third axis, the min class, the first and the last blocking
 * voxel and the number of blocking voxels -- on the host se::Octree snapshot that DenseSLAMSystem::getMap() materialises: the executable
 * definition of se_hip_project_columns (include/se_hip.h), without Eigen, beside clearance.hpp.
 *
 * The columns run along `axis` (coordinate w).  The two remaining axes in ascending order are u (the fastest output index) and v:
 *     axis 2: u = x, v = y;   axis 1: u = x, v = z;   axis 0: u = y, v = z.
 * Cell (l, j, i) is the set of voxels with u = lo[0] + i, v = lo[1] + j and w in [a_l, b_l).  A voxel of [0, size)^3 has the class
 * test(Octree::get(voxel)), every other voxel of Z^3 is unseen, and a voxel blocks when its class is <= stop_at.  Per cell:
 *     status = the min class over its voxels (occupied < unseen < empty, as collision_status orders them),
 *     first / last = the smallest / largest w of a blocking voxel (project_none if there is none), count = how many block.
 * A stretch [r0, r1) of one class c folds as  status = min(status, c)  and, if c blocks,  first = min(first, r0), last = max(last, r1 - 1),
 * count += r1 - r0  (fold_run): that is all the traversal and the device do with an absent octant or with the outside of the volume.
 *
 * Three things are provided:
 *   project_valid / project_uvw / fold_run   the formulas;
 *   project_columns(map, request, test)      per column a walk up [a, b) ∩ [0, size) in octant steps: the descent of Octree::get at w ends
 *                                            at a block (its up to 8 voxels are read) or at an absent child of side s, whose value_[child]
 *                                            answers [w0, w0 + s) ∩ [a, b) -- exact, every voxel of that octant reads that value; the
 *                                            parts outside the volume in closed form;
 *   project_columns_brute(map, ...)          the definition, literally: every voxel of every cell through Octree::get.  This is the model
 *                                            the traversal and the device are held to.
 */
#ifndef SE_HIP_PROJECT_COLUMNS_HPP
#define SE_HIP_PROJECT_COLUMNS_HPP

#include <cstdint>
#include <vector>

#include "octree.hpp"
#include "octree_collision.hpp"

namespace se {
namespace geometry {

constexpr int project_limit = 1 << 20;       /* |coordinate| bound of lo, lo + side, a and b of a valid request */
constexpr int project_max_layers = 16;
constexpr int64_t project_max_cells = (int64_t)1 << 28;
constexpr int project_none = INT32_MIN;      /* first / last of a cell without a blocking voxel: SE_HIP_PROJECT_NONE */

struct project_request {
  int axis;
  int lo[2], side[2];   /* u, v */
  int n_layers;
  int layers[project_max_layers][2];
  collision_status stop_at;
};

struct project_cell {
  collision_status status;
  int first, last, count;
};

inline bool project_valid(const project_request& r) {
  if (r.axis < 0 || r.axis > 2) return false;
  if (r.stop_at != collision_status::occupied && r.stop_at != collision_status::unseen) return false;
  if (r.n_layers < 1 || r.n_layers > project_max_layers) return false;
  auto in = [](int64_t v) { return v >= -project_limit && v <= project_limit; };
  for (int k = 0; k < 2; ++k)
    if (r.side[k] < 1 || !in(r.lo[k]) || !in((int64_t)r.lo[k] + r.side[k])) return false;
  for (int l = 0; l < r.n_layers; ++l)
    if (!in(r.layers[l][0]) || !in(r.layers[l][1]) || r.layers[l][0] >= r.layers[l][1]) return false;
  return (int64_t)r.n_layers * r.side[0] * r.side[1] <= project_max_cells;
}

/* (u, v, w) of a request along `axis` as (x, y, z) */
inline int3 project_uvw(const int axis, const int u, const int v, const int w) {
  if (axis == 2) return {{u, v, w}};
  if (axis == 1) return {{u, w, v}};
  return {{w, u, v}};
}

inline project_cell project_empty_cell() { return {collision_status::empty, project_none, project_none, 0}; }

/* the stretch [r0, r1) of class c */
inline void fold_run(project_cell& cell, const collision_status c, const collision_status stop_at, const int r0, const int r1) {
  if (r0 >= r1) return;
  if ((int)c < (int)cell.status) cell.status = c;
  if ((int)c <= (int)stop_at) {
    if (cell.count == 0 || r0 < cell.first) cell.first = r0;
    if (cell.count == 0 || r1 - 1 > cell.last) cell.last = r1 - 1;
    cell.count += r1 - r0;
  }
}

/* The traversal: one column (u, v), interval [a, b). */
template <typename T, typename TestF>
project_cell project_column(const Octree<T>& map, const int axis, const int u, const int v, const int a, const int b, TestF test, const collision_status stop_at) {
  project_cell cell = project_empty_cell();
  const int n = map.size(), bs = (int)VoxelBlock<T>::side;
  if (u < 0 || u >= n || v < 0 || v >= n) {   /* the whole column lies outside the volume */
    fold_run(cell, collision_status::unseen, stop_at, a, b);
    return cell;
  }
  fold_run(cell, collision_status::unseen, stop_at, a, b < 0 ? b : 0);
  const int end = b < n ? b : n;
  int w = a > 0 ? a : 0;
  while (w < end) {
    const int3 p = project_uvw(axis, u, v, w);
    Node<T>* node = map.root();
    if (!node) {   /* Octree::get without a root */
      fold_run(cell, test(voxel_traits<T>::initValue()), stop_at, w, end);
      break;
    }
    int s = n;   /* side of `node` */
    bool answered = false;
    while (s > bs) {
      const int h = s / 2;
      const int id = ((p(0) & h) > 0) + 2 * ((p(1) & h) > 0) + 4 * ((p(2) & h) > 0);
      Node<T>* child = node->child(id);
      if (!child) {   /* the absent octant of side h that holds w: [w0, w0 + h) along the axis */
        const int w1 = (w & ~(h - 1)) + h;
        fold_run(cell, test(node->value_[id]), stop_at, w, w1 < end ? w1 : end);
        w = w1;
        answered = true;
        break;
      }
      node = child;
      s = h;
    }
    if (answered) continue;
    const VoxelBlock<T>* block = static_cast<const VoxelBlock<T>*>(node);
    const int w1 = (w & ~(bs - 1)) + bs;
    for (; w < w1 && w < end; ++w) {
      const int3 q = project_uvw(axis, u, v, w);
      fold_run(cell, test(block->data(q(0), q(1), q(2))), stop_at, w, w + 1);
    }
  }
  fold_run(cell, collision_status::unseen, stop_at, a > n ? a : n, b);
  return cell;
}

/* The definition: one column, every voxel through Octree::get. */
template <typename T, typename TestF>
project_cell project_column_brute(const Octree<T>& map, const int axis, const int u, const int v, const int a, const int b, TestF test, const collision_status stop_at) {
  project_cell cell = project_empty_cell();
  const int n = map.size();
  for (int w = a; w < b; ++w) {
    const int3 p = project_uvw(axis, u, v, w);
    const bool in = p(0) >= 0 && p(1) >= 0 && p(2) >= 0 && p(0) < n && p(1) < n && p(2) < n;
    const collision_status c = in ? test(map.get(p(0), p(1), p(2))) : collision_status::unseen;
    if ((int)c < (int)cell.status) cell.status = c;
    if ((int)c <= (int)stop_at) {
      if (cell.count == 0) cell.first = w;
      cell.last = w;
      ++cell.count;
    }
  }
  return cell;
}

/* All cells of a request, [L][side_v][side_u]; empty for an invalid request. */
template <typename T, typename TestF>
std::vector<project_cell> project_columns(const Octree<T>& map, const project_request& r, TestF test) {
  std::vector<project_cell> out;
  if (!project_valid(r)) return out;
  out.reserve((size_t)r.n_layers * r.side[0] * r.side[1]);
  for (int l = 0; l < r.n_layers; ++l)
    for (int j = 0; j < r.side[1]; ++j)
      for (int i = 0; i < r.side[0]; ++i) out.push_back(project_column(map, r.axis, r.lo[0] + i, r.lo[1] + j, r.layers[l][0], r.layers[l][1], test, r.stop_at));
  return out;
}
template <typename T, typename TestF>
std::vector<project_cell> project_columns_brute(const Octree<T>& map, const project_request& r, TestF test) {
  std::vector<project_cell> out;
  if (!project_valid(r)) return out;
  out.reserve((size_t)r.n_layers * r.side[0] * r.side[1]);
  for (int l = 0; l < r.n_layers; ++l)
    for (int j = 0; j < r.side[1]; ++j)
      for (int i = 0; i < r.side[0]; ++i)
        out.push_back(project_column_brute(map, r.axis, r.lo[0] + i, r.lo[1] + j, r.layers[l][0], r.layers[l][1], test, r.stop_at));
  return out;
}

}  // namespace geometry
}  // namespace se

#endif /* SE_HIP_PROJECT_COLUMNS_HPP */
