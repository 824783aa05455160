// Batched collision queries for axis-aligned boxes against the resident map (se_hip_collide_boxes, include/se_hip.h): for N boxes in voxel
// units, what the reference's se::geometry::collides_with (se_core/include/se/geometry/octree_collision.hpp:74-167) answers -- exactly
// (SE_HIP_COLLIDE_REFERENCE), or as the min over the box's voxels of classify(Octree::get(v)) (SE_HIP_COLLIDE_STRICT).
//
// One wave64 per box (grid-stride over int64 n), wave-uniform control flow, on the frontier descent of se_frontier.h; the frontier holds
// the present overlapping octants.  Its loops are bounded by the structure, as argued there.
//   - at the leaf level the 64 lanes cover the 8 x 8 columns of one block, each lane the box's z range of its column (loads unrolled).
// STRICT folds classify(value_[child]) of every overlapping absent child and the voxels of every overlapping present block, plus unseen for a
// box that leaves the volume; it stops at the first occupied step.
// REFERENCE evaluates the closed form of the reference's DFS: leaf steps meet the hit blocks in ascending Morton order, so
// the first leaf step with a hit yields L* (its lowest lane), the events ev(Q) = classify(Q.value_[0]) of expanded nodes count when Q's
// octant ends at or before code(L*), and the search stops there.
// Per step, the events of one class come from nodes of one level in ascending lane order, so the lowest lane carries the smallest end.
#pragma once
#include "se_frontier.h"

#define SE_WG_COLLIDE 64                // one wave per workgroup
#define SE_COLLIDE_LIMIT (1 << 30)      // lo and lo + side within [-2^30, 2^30], else the box is invalid
#define SE_COLLIDE_OCC 0u
#define SE_COLLIDE_UNSEEN 1u
#define SE_COLLIDE_EMPTY 2u
#define SE_COLLIDE_INVALID 255u

struct CollideArgs { const int32_t* boxes; long long n; uint8_t* status; float thr; int above; int reference; };

__device__ __forceinline__ uint32_t se_collide_class(float x, float y, const FieldConst fc, float thr, int above) {
  if (x == fc.init_x && y == fc.init_y) return SE_COLLIDE_UNSEEN;
  return (above ? x > thr : x < thr) ? SE_COLLIDE_OCC : SE_COLLIDE_EMPTY;
}

// min of the lanes' classes (inactive lanes pass EMPTY)
__device__ __forceinline__ uint32_t se_collide_wave_min(uint32_t c) {
  if (__ballot(c == SE_COLLIDE_OCC) != 0ull) return SE_COLLIDE_OCC;
  return __ballot(c == SE_COLLIDE_UNSEEN) != 0ull ? SE_COLLIDE_UNSEEN : SE_COLLIDE_EMPTY;
}

// The voxels of the block at slot `slot` (corner bc) inside the half-open range [r0, r1) per axis (already clipped to the block), folded
// from empty.  Lane = column (x, y) of the block, z unrolled so that the loads of a column are in flight together.
__device__ __forceinline__ uint32_t se_collide_block(const DevMap& m, const FieldConst fc, float thr, int above, uint32_t slot, int bcx, int bcy, int bcz,
                                                     int r0x, int r1x, int r0y, int r1y, int r0z, int r1z) {
  const int lane = (int)(threadIdx.x & 63u);
  const int x = bcx + (lane & 7), y = bcy + (lane >> 3);
  const bool col = x >= r0x && x < r1x && y >= r0y && y < r1y;
  uint32_t c = SE_COLLIDE_EMPTY;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int z = bcz + k;
    if (col && z >= r0z && z < r1z) {
      const size_t vi = se_brick_voxel(slot, k);
      c = min(c, se_collide_class(m.vx[vi], se_ld_y(m, vi), fc, thr, above));
    }
  }
  return se_collide_wave_min(c);
}

// inclusive midpoint overlap of the reference (aabb_collision.hpp axis_overlap) for a box (amid = lo + side/2, edge ae) and an octant
// (corner c, side s), in 64-bit so that ae + s cannot overflow
__device__ __forceinline__ bool se_collide_ref_overlap(long long amid, long long ae, int c, int s) {
  const long long d = (long long)(c + s / 2) - amid;
  return (d < 0 ? -d : d) <= (ae + s) / 2;
}

template <bool DENSE>
__global__ __launch_bounds__(SE_WG_COLLIDE) void k_collide_boxes(DevMap m, CollideArgs a) {
  __shared__ SeFrontier f;
  const FieldConst fc = se_field_const(m);
  const int lane = (int)(threadIdx.x & 63u);
  se_frontier_init(f, m);
  const int leaf = m.leaf_level;
  const float thr = a.thr;
  const int above = a.above;

  for (long long i = blockIdx.x; i < a.n; i += gridDim.x) {
    const int32_t* bx = a.boxes + 6 * i;
    const int lo[3] = {bx[0], bx[1], bx[2]}, sd[3] = {bx[3], bx[4], bx[5]};
    bool valid = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const long long hi = (long long)lo[k] + sd[k];
      valid = valid && sd[k] >= 1 && lo[k] >= -SE_COLLIDE_LIMIT && lo[k] <= SE_COLLIDE_LIMIT && hi >= -SE_COLLIDE_LIMIT && hi <= SE_COLLIDE_LIMIT;
    }
    uint32_t st = SE_COLLIDE_EMPTY;
    if (!valid) st = SE_COLLIDE_INVALID;
    // STRICT: the box clipped to the volume, [b0, b1) per axis; REFERENCE: midpoint and edge of the box
    int b0[3], b1[3];
    long long amid[3], ae[3];
    bool run = valid;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      b0[k] = max(lo[k], 0);
      b1[k] = (int)min((long long)lo[k] + sd[k], (long long)m.size);
      amid[k] = (long long)lo[k] + sd[k] / 2;
      ae[k] = sd[k];
      if (valid && !a.reference) {
        if (lo[k] < 0 || (long long)lo[k] + sd[k] > m.size) st = SE_COLLIDE_UNSEEN;   // a part outside the volume
        if (b0[k] >= b1[k]) run = false;                                             // nothing inside it
      }
    }
    // REFERENCE bookkeeping: per class, the smallest end (block-unit Morton code) of an expanded node that raised it; L* found
    uint32_t end_cls[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    bool found = false;
    int l;
    SeFrontierStep t;
    se_frontier_root(f, l);
    while (run && se_frontier_pop(f, m, l, t)) {
      const int s = t.s, cx = t.cx, cy = t.cy, cz = t.cz;
      // (REFERENCE needs `present` of all eight children of a parent, overlapping or not)
      const uint32_t e = se_frontier_entry(f, m, t, t.live);
      const bool present = t.live && e != 0u && e != SE_PENDING;
      bool ov;
      if (a.reference) {
        ov = se_collide_ref_overlap(amid[0], ae[0], cx * s, s) && se_collide_ref_overlap(amid[1], ae[1], cy * s, s) && se_collide_ref_overlap(amid[2], ae[2], cz * s, s);
      } else {
        ov = cx * s < b1[0] && cx * s + s > b0[0] && cy * s < b1[1] && cy * s + s > b0[1] && cz * s < b1[2] && cz * s + s > b0[2];
      }
      ov = ov && t.live;
      // events of absent overlapping children
      const bool absent = ov && !present;
      if (!a.reference) {
        uint32_t cls = SE_COLLIDE_EMPTY;
        if (absent) cls = se_collide_class(m.nx[(size_t)t.nid * 8 + t.c], m.ny[(size_t)t.nid * 8 + t.c], fc, thr, above);
        st = min(st, se_collide_wave_min(cls));
      } else {
        const unsigned long long has = __ballot(present);   // children_mask_ != 0 of each parent: its 8-lane group
        const bool ev = absent && ((has >> (8 * t.j)) & 0xFFull) != 0ull;
        uint32_t cls = SE_COLLIDE_EMPTY + 1u;
        if (ev) cls = se_collide_class(m.nx[(size_t)t.nid * 8], m.ny[(size_t)t.nid * 8], fc, thr, above);
        const int sh = 3 * (leaf - t.L + 1);   // the parent, a level-(L - 1) octant, spans 8^(leaf - L + 1) block codes
        const uint32_t end = (morton30((int)(t.pp & 1023u), (int)((t.pp >> 10) & 1023u), (int)(t.pp >> 20)) + 1u) << sh;
#pragma unroll
        for (uint32_t k = 0; k < 3; ++k) {
          const unsigned long long b = __ballot(cls == k);
          if (b) {   // the lowest lane: the parent of smallest code among those that raised class k in this step
            const uint32_t e0 = (uint32_t)__builtin_amdgcn_readlane((int)end, (int)__builtin_ctzll(b));
            end_cls[k] = min(end_cls[k], e0);
          }
        }
      }
      const bool hit = ov && present;
      if (t.L < leaf) {
        se_frontier_push(f, t, hit, e, l);
      } else {
        __syncthreads();   // the leaf step's barrier (se_frontier.h)
        unsigned long long b = __ballot(hit);
        int qx, qy, qz;
        if (a.reference) {
          if (b) {   // L* = the lowest lane: its voxels that pass the inclusive test, folded from empty
            const uint32_t slot = se_frontier_block<DENSE>(m, t, e, (int)__builtin_ctzll(b), qx, qy, qz);
            int r0[3], r1[3];
            const int q[3] = {qx * 8, qy * 8, qz * 8};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
              const long long h = (ae[k] + 1) / 2;   // voxel (edge 1) overlap: |v - amid| <= (ae + 1) / 2
              r0[k] = (int)max(amid[k] - h, (long long)q[k]);
              r1[k] = (int)min(amid[k] + h + 1, (long long)q[k] + 8);
            }
            const uint32_t code = morton30(qx, qy, qz);
            st = se_collide_block(m, fc, thr, above, slot, q[0], q[1], q[2], r0[0], r1[0], r0[1], r1[1], r0[2], r1[2]);
#pragma unroll
            for (uint32_t k = 0; k < 3; ++k)
              if (end_cls[k] <= code) st = min(st, k);
            found = true;
            break;
          }
        } else {
          while (b && st != SE_COLLIDE_OCC) {
            const int w = (int)__builtin_ctzll(b);
            b &= b - 1ull;
            const uint32_t slot = se_frontier_block<DENSE>(m, t, e, w, qx, qy, qz);
            st = min(st, se_collide_block(m, fc, thr, above, slot, qx * 8, qy * 8, qz * 8, max(b0[0], qx * 8), min(b1[0], qx * 8 + 8),
                                          max(b0[1], qy * 8), min(b1[1], qy * 8 + 8), max(b0[2], qz * 8), min(b1[2], qz * 8 + 8)));
          }
        }
      }
      if (!a.reference && st == SE_COLLIDE_OCC) break;   // nothing beats occupied
    }
    if (valid && a.reference && !found) {
#pragma unroll
      for (uint32_t k = 0; k < 3; ++k)
        if (end_cls[k] != 0xFFFFFFFFu) st = min(st, k);
    }
    if (lane == 0) a.status[i] = (uint8_t)st;
  }
}
