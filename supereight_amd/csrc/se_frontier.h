// The descent of the wave-per-query octree kernels (k_collide_boxes, k_collide_motions, k_clearance_boxes): one wave64 per query walks the
// index pyramid tab[] from the root and never enters an absent octant (SE_PENDING counts as absent, as in k_query_points; occ[] is not read,
// so its lazy commit does not matter).  This header owns the traversal and knows nothing about any query: what a kernel keeps, folds and
// prunes is decided in its own loop, between these calls.
//
//   SeFrontier f (LDS)      a frontier of kept present octants per level
//   se_frontier_init        once per kernel
//   se_frontier_root        once per query: the frontier holds the root alone
//   se_frontier_pop         a step: up to 8 nodes of the deepest non-empty level, their 64 children one per lane (SeFrontierStep)
//   se_frontier_entry       the child's index entry, loaded for the lanes the kernel names
//   se_frontier_push        (child level above the blocks) the kernel's kept present children go into the next level
//   se_frontier_block       (child level = blocks) one kept block's position and brick slot, broadcast to the wave
//
// 64 entries per level suffice: a step always takes the deepest non-empty level, so the level below it is empty when the step fills it, and
// a step pushes at most 64 children.
// Order: push compacts a step's children in descending Morton order and pop takes from the end, lane group j the j-th last.  Within a step
// the lanes therefore run in ascending Morton order, and the pending octants of a deeper level always precede (in Morton order) those of a
// shallower one: leaf steps meet the kept blocks in ascending Morton order.  REFERENCE mode of the box query rests on that.
// Every loop ends: a step pops at least one entry and pushes only children of what it popped, and the pyramid is finite; pop's walk to the
// deepest non-empty level stops at level 0; a leaf step offers at most 64 blocks.
// Barriers (one wave per workgroup: they order the LDS traffic): root resets between two, so that neither the last query's reads nor this
// one's first pop cross it; pop has one between reading the entries and lowering the count; push has one between writing the entries and
// publishing their count and one after it.  A leaf step does not push: the kernel places the one __syncthreads() that publishes pop's
// lowered count before the next pop.
#pragma once
#include "se_kernels.h"

struct SeFrontier {
  uint32_t pos[SE_MAX_LEVELS][64];   // packed octant position (x | y << 10 | z << 20) in units of the level's octants, descending Morton order
  uint32_t nid[SE_MAX_LEVELS][64];   // ... and its node id
  uint32_t off[SE_MAX_LEVELS];       // m.off[] (a by-value DevMap array indexed by a runtime level would go to scratch)
  int cnt[SE_MAX_LEVELS];
};

// What a lane holds in a step: child c of the j-th popped parent (live iff there is a j-th).
struct SeFrontierStep {
  bool live;
  int j, c;
  int L, s;          // the child's level and side in voxels
  int cx, cy, cz;    // the child's position in units of s
  uint32_t pp, nid;  // the parent's packed position and node id
};

__device__ __forceinline__ void se_frontier_init(SeFrontier& f, const DevMap& m) {
  const int lane = (int)(threadIdx.x & 63u);
#pragma unroll
  for (int l = 0; l < SE_MAX_LEVELS; ++l)
    if (lane == l) f.off[l] = m.off[l];
}

// l: the level the next pop looks at first
__device__ __forceinline__ void se_frontier_root(SeFrontier& f, int& l) {
  __syncthreads();
  if ((threadIdx.x & 63u) == 0u) {
    f.pos[0][0] = 0u; f.nid[0][0] = 0u;
#pragma unroll
    for (int k = 0; k < SE_MAX_LEVELS; ++k) f.cnt[k] = k == 0 ? 1 : 0;
  }
  __syncthreads();
  l = 0;
}

// false: the frontier is empty (t is cleared).  Else up to 8 entries leave the end of the deepest non-empty level (l on return) and t is filled.
__device__ __forceinline__ bool se_frontier_pop(SeFrontier& f, const DevMap& m, int& l, SeFrontierStep& t) {
  int cnt;
  while ((cnt = f.cnt[l]) == 0) {
    if (l == 0) { t = SeFrontierStep{}; return false; }   // (cleared: left as it was, the last step stays live in registers round the query loop)
    --l;
  }
  const int lane = (int)(threadIdx.x & 63u);
  const int take = min(cnt, 8);
  t.j = lane >> 3; t.c = lane & 7;
  t.live = t.j < take;
  t.pp = t.live ? f.pos[l][cnt - 1 - t.j] : 0u;
  t.nid = t.live ? f.nid[l][cnt - 1 - t.j] : 0u;
  __syncthreads();
  if (lane == 0) f.cnt[l] = cnt - take;
  t.L = l + 1;
  t.s = m.size >> t.L;
  t.cx = (int)((t.pp & 1023u) << 1) | (t.c & 1);
  t.cy = (int)(((t.pp >> 10) & 1023u) << 1) | ((t.c >> 1) & 1);
  t.cz = (int)((t.pp >> 20) << 1) | (t.c >> 2);
  return true;
}

// the index entry of the lane's child if `load` (which implies t.live), else 0
__device__ __forceinline__ uint32_t se_frontier_entry(const SeFrontier& f, const DevMap& m, const SeFrontierStep& t, bool load) {
  return load ? m.tab[f.off[t.L] + (((((uint32_t)t.cz << t.L) | (uint32_t)t.cy) << t.L) | (uint32_t)t.cx)] : 0u;
}

// The lanes with `hit` (present children, index entry e) become level t.L, in descending Morton order; l follows them down if there are any.
__device__ __forceinline__ void se_frontier_push(SeFrontier& f, const SeFrontierStep& t, bool hit, uint32_t e, int& l) {
  const unsigned long long b = __ballot(hit);
  const int tot = __popcll(b);
  if (hit) {
    const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
    f.pos[t.L][tot - 1 - (int)rank] = pack_pos(t.cx, t.cy, t.cz);
    f.nid[t.L][tot - 1 - (int)rank] = e - 1u;
  }
  __syncthreads();
  if ((threadIdx.x & 63u) == 0u && tot) f.cnt[t.L] = tot;
  __syncthreads();
  if (tot) l = t.L;
}

// Lane w's child is a block: its position in blocks to every lane, and its brick slot -- the dense grid addresses a block's brick by its grid
// position, the pooled one by its index entry e.
template <bool DENSE>
__device__ __forceinline__ uint32_t se_frontier_block(const DevMap& m, const SeFrontierStep& t, uint32_t e, int w, int& qx, int& qy, int& qz) {
  qx = __builtin_amdgcn_readlane(t.cx, w); qy = __builtin_amdgcn_readlane(t.cy, w); qz = __builtin_amdgcn_readlane(t.cz, w);
  return DENSE ? block_linear(m, qx, qy, qz) : (uint32_t)__builtin_amdgcn_readlane((int)e, w) - 1u;
}

// The float index of the lane's voxel in slice k of the brick at `slot`, for the block folds: lane = x + 8 y, its column of the block.
__device__ __forceinline__ size_t se_brick_voxel(uint32_t slot, int k) {
  return (size_t)slot * SE_BRICK_STRIDE + (size_t)((threadIdx.x & 63u) + ((uint32_t)k << 6));
}
