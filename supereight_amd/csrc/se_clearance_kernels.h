// Batched clearance queries against the resident map (se_hip_clearance_boxes, include/se_hip.h): for N boxes in voxel units, the squared
// Euclidean distance from the box [lo, lo + side) to the nearest blocking voxel within r_max, and that voxel -- among the nearest ones the
// smallest in (z, y, x) order.  A voxel v blocks when classify(Octree::get(v)) <= stop_at (outside the volume: unseen).  The host
// restatement and the literal definition are include/se/clearance.hpp.
//
// Everything is integer arithmetic.  The gap of a cube (corner c, side s) on axis k is g_k = max(0, c_k - hi_k, lo_k - c_k - s), hi = lo + side,
// and its distance d2 = g_x^2 + g_y^2 + g_z^2.  The voxels of the cube that attain the cube's d2 are a product of per-axis intervals, so the
// smallest of them in (z, y, x) order has, per axis, the interval's lowest coordinate: c if the cube lies above the box, c + s - 1 if it
// lies below, max(lo - 1, c) otherwise.  An answer is the pair (d2, key), key = (z, y, x) packed into 63 bits (each coordinate + 2^20 in 21
// bits: a valid query has lo, hi within [-2^19, 2^19] and r_max <= 32767, so a witness lies within +-2^20 and d2 < 2^30); pairs are compared
// lexicographically.  Every voxel of a cube has a pair not smaller than the cube's own (its d2 with the key of its lowest nearest voxel), so
// skipping an octant whose pair is not smaller than the best found so far loses nothing -- not even a witness of equal distance and smaller
// key.  The best starts at (r_max^2, no key), which also keeps everything beyond r_max out.  Gaps are clamped to 32768 (anything beyond
// r_max is beyond) and squared in uint32: three such squares stay below 2^32.
//
// One wave64 per query (grid-stride over int64 n), wave-uniform control flow, on the frontier descent of se_frontier.h; the frontier holds
// the present octants whose pair is below the best.
//   - an absent kept child whose classify(value_[child]) blocks is a candidate as a whole cube, with the cube's pair: exact, because every
//     voxel of the octant reads that value;
//   - at a block the lanes are its 8 x 8 columns: a lane forms the x / y part of its column's distance once and then tests its 8 z voxels
//     (loads unrolled, in flight together; only voxels whose pair could still win are loaded);
//   - each lane keeps its best pair; the wave minimum is taken after a step in which some lane improved: the uniform best is what pruning
//     reads and what is written;
//   - the voxels outside the volume (they block only with stop_at unseen) are six half-spaces with a closed form each, folded in before the
//     descent.
// Every loop is bounded by the structure: the descent by the argument in se_frontier.h, whatever the test, and a leaf step visits at most
// 64 blocks.
#pragma once
#include "se_collide_kernels.h"

#define SE_CLEAR_LIMIT (1 << 19)        // lo and lo + side within [-2^19, 2^19], else the query is invalid
#define SE_CLEAR_RMAX 32767             // r_max within [0, 32767], else the query is invalid
#define SE_CLEAR_GAP_MAX 32768          // a gap is clamped here: beyond every r_max
#define SE_CLEAR_BIAS (1 << 20)         // added to a witness coordinate in the packed key
#define SE_CLEAR_NONE (-1)
#define SE_CLEAR_INVALID (-2)
#define SE_CLEAR_NO_KEY 0xFFFFFFFFFFFFFFFFull

struct ClearanceArgs { const int32_t* queries; long long n; int32_t* d2; int32_t* nearest; float thr; int above; uint32_t stop_at; };

// the gap on one axis between the box [lo, hi) and the cube [c, c + s), clamped
__device__ __forceinline__ uint32_t se_clear_gap(int lo, int hi, int c, int s) { return (uint32_t)min(max(max(c - hi, lo - c - s), 0), SE_CLEAR_GAP_MAX); }
// the lowest coordinate of the cube's voxels that attain that gap
__device__ __forceinline__ int se_clear_low(int lo, int hi, int c, int s) { return c >= hi ? c : (c + s <= lo ? c + s - 1 : max(lo - 1, c)); }
__device__ __forceinline__ unsigned long long se_clear_key(int x, int y, int z) {
  return ((unsigned long long)(uint32_t)(z + SE_CLEAR_BIAS) << 42) | ((unsigned long long)(uint32_t)(y + SE_CLEAR_BIAS) << 21) | (unsigned long long)(uint32_t)(x + SE_CLEAR_BIAS);
}
// (d, k) < (bd, bk), lexicographically
__device__ __forceinline__ bool se_clear_less(uint32_t d, unsigned long long k, uint32_t bd, unsigned long long bk) { return d < bd || (d == bd && k < bk); }

// If some lane improved its best (bd, bk): the wave's smallest pair into every lane's best and into the uniform (gd, gk).
__device__ __forceinline__ void se_clear_settle(uint32_t& bd, unsigned long long& bk, bool& improved, uint32_t& gd, unsigned long long& gk) {
  if (__ballot(improved) == 0ull) return;
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    const uint32_t od = (uint32_t)__shfl_xor((int)bd, off);
    const uint32_t ol = (uint32_t)__shfl_xor((int)(uint32_t)bk, off), oh = (uint32_t)__shfl_xor((int)(uint32_t)(bk >> 32), off);
    const unsigned long long ok = ((unsigned long long)oh << 32) | ol;
    if (se_clear_less(od, ok, bd, bk)) { bd = od; bk = ok; }
  }
  gd = bd = (uint32_t)__builtin_amdgcn_readfirstlane((int)bd);
  gk = bk = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(bk >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)bk);
  improved = false;
}

// The voxels of the block at slot `slot` (corner bc) whose pair is below the lane's best (bd, bk) and which block: folded into that best.
// Lane = column (x, y) of the block.
__device__ __forceinline__ void se_clear_block(const DevMap& m, const FieldConst fc, float thr, int above, uint32_t stop_at, uint32_t slot, int bcx, int bcy, int bcz,
                                               const int* lo, const int* hi, uint32_t& bd, unsigned long long& bk, bool& improved) {
  const int lane = (int)(threadIdx.x & 63u);
  const int x = bcx + (lane & 7), y = bcy + (lane >> 3);
  const uint32_t gx = se_clear_gap(lo[0], hi[0], x, 1), gy = se_clear_gap(lo[1], hi[1], y, 1);
  const uint32_t dxy = gx * gx + gy * gy;
  const unsigned long long kxy = se_clear_key(x, y, -SE_CLEAR_BIAS);
  bool t[8];
  uint32_t dz[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint32_t gz = se_clear_gap(lo[2], hi[2], bcz + k, 1);
    dz[k] = dxy + gz * gz;
    t[k] = se_clear_less(dz[k], kxy | ((unsigned long long)(uint32_t)(bcz + k + SE_CLEAR_BIAS) << 42), bd, bk);
  }
  float vx[8], vy[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    vx[k] = fc.init_x; vy[k] = fc.init_y;
    if (t[k]) {
      const size_t vi = se_brick_voxel(slot, k);
      vx[k] = m.vx[vi]; vy[k] = se_ld_y(m, vi);
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (t[k] && se_collide_class(vx[k], vy[k], fc, thr, above) <= stop_at) {
      const unsigned long long key = kxy | ((unsigned long long)(uint32_t)(bcz + k + SE_CLEAR_BIAS) << 42);
      if (se_clear_less(dz[k], key, bd, bk)) { bd = dz[k]; bk = key; improved = true; }
    }
  }
}

template <bool DENSE>
__global__ __launch_bounds__(SE_WG_COLLIDE) void k_clearance_boxes(DevMap m, ClearanceArgs a) {
  __shared__ SeFrontier f;
  const FieldConst fc = se_field_const(m);
  const int lane = (int)(threadIdx.x & 63u);
  se_frontier_init(f, m);
  const int leaf = m.leaf_level;
  const float thr = a.thr;
  const int above = a.above;
  const uint32_t stop_at = a.stop_at;

  for (long long i = blockIdx.x; i < a.n; i += gridDim.x) {
    const int32_t* q = a.queries + 7 * i;
    int lo[3], hi[3];
    bool valid = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const long long l0 = q[k], sd = q[3 + k];
      const long long h0 = l0 + sd;
      valid = valid && sd >= 1 && l0 >= -SE_CLEAR_LIMIT && l0 <= SE_CLEAR_LIMIT && h0 >= -SE_CLEAR_LIMIT && h0 <= SE_CLEAR_LIMIT;
      lo[k] = (int)l0; hi[k] = (int)h0;
    }
    const int r_max = q[6];
    valid = valid && r_max >= 0 && r_max <= SE_CLEAR_RMAX;
    // the wave's best pair so far: (r_max^2, no key) admits exactly the pairs with d2 <= r_max^2
    uint32_t gd = valid ? (uint32_t)(r_max * r_max) : 0u;
    unsigned long long gk = SE_CLEAR_NO_KEY;
    if (valid && stop_at >= SE_COLLIDE_UNSEEN) {
      // the voxels outside the volume, all unseen: per half-space v_k <= -1 / v_k >= size its nearest voxels' pair
#pragma unroll
      for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int up = 0; up < 2; ++up) {
          const uint32_t g = (uint32_t)min(max(up ? m.size - hi[k] : lo[k], 0), SE_CLEAR_GAP_MAX);
          int w[3] = {lo[0] - 1, lo[1] - 1, lo[2] - 1};
          w[k] = up ? max(lo[k] - 1, m.size) : min(lo[k] - 1, -1);
          const unsigned long long key = se_clear_key(w[0], w[1], w[2]);
          if (se_clear_less(g * g, key, gd, gk)) { gd = g * g; gk = key; }
        }
      }
    }
    bool run = valid;
    if (valid) {   // nothing inside the volume can win: no descent
      const uint32_t g0 = se_clear_gap(lo[0], hi[0], 0, m.size), g1 = se_clear_gap(lo[1], hi[1], 0, m.size), g2 = se_clear_gap(lo[2], hi[2], 0, m.size);
      run = se_clear_less(g0 * g0 + g1 * g1 + g2 * g2, se_clear_key(se_clear_low(lo[0], hi[0], 0, m.size), se_clear_low(lo[1], hi[1], 0, m.size), se_clear_low(lo[2], hi[2], 0, m.size)), gd, gk);
    }
    uint32_t bd = gd;             // this lane's best; equal to the wave's after each step
    unsigned long long bk = gk;
    bool improved = false;
    int l;
    SeFrontierStep t;
    se_frontier_root(f, l);
    while (run && se_frontier_pop(f, m, l, t)) {
      const int s = t.s, cx = t.cx, cy = t.cy, cz = t.cz;
      // the child octant's pair: its distance and the key of its lowest nearest voxel
      const uint32_t g0 = se_clear_gap(lo[0], hi[0], cx * s, s), g1 = se_clear_gap(lo[1], hi[1], cy * s, s), g2 = se_clear_gap(lo[2], hi[2], cz * s, s);
      const uint32_t cd = g0 * g0 + g1 * g1 + g2 * g2;
      const unsigned long long ck = se_clear_key(se_clear_low(lo[0], hi[0], cx * s, s), se_clear_low(lo[1], hi[1], cy * s, s), se_clear_low(lo[2], hi[2], cz * s, s));
      const bool keep = t.live && se_clear_less(cd, ck, gd, gk);
      const uint32_t e = se_frontier_entry(f, m, t, keep);
      const bool present = keep && e != 0u && e != SE_PENDING;
      // absent kept children: the whole octant has the class of value_[child]
      if (keep && !present) {
        const uint32_t cls = se_collide_class(m.nx[(size_t)t.nid * 8 + t.c], m.ny[(size_t)t.nid * 8 + t.c], fc, thr, above);
        if (cls <= stop_at && se_clear_less(cd, ck, bd, bk)) { bd = cd; bk = ck; improved = true; }
      }
      const bool hit = keep && present;
      if (t.L < leaf) {
        se_frontier_push(f, t, hit, e, l);
      } else {
        __syncthreads();   // the leaf step's barrier (se_frontier.h)
        se_clear_settle(bd, bk, improved, gd, gk);   // absent siblings of this step may already beat some of its blocks
        unsigned long long b = __ballot(hit);
        while (b) {
          const int w = (int)__builtin_ctzll(b);
          b &= b - 1ull;
          // the best may have improved since this block passed the test above
          const uint32_t wd = (uint32_t)__builtin_amdgcn_readlane((int)cd, w);
          const unsigned long long wk = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(ck >> 32), w) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)ck, w);
          if (!se_clear_less(wd, wk, gd, gk)) continue;
          int qx, qy, qz;
          const uint32_t slot = se_frontier_block<DENSE>(m, t, e, w, qx, qy, qz);
          se_clear_block(m, fc, thr, above, stop_at, slot, qx * 8, qy * 8, qz * 8, lo, hi, bd, bk, improved);
          se_clear_settle(bd, bk, improved, gd, gk);
        }
      }
      se_clear_settle(bd, bk, improved, gd, gk);
    }
    if (lane == 0) {
      const bool found = valid && gk != SE_CLEAR_NO_KEY;
      a.d2[i] = !valid ? SE_CLEAR_INVALID : (found ? (int32_t)gd : SE_CLEAR_NONE);
      if (a.nearest) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
          a.nearest[3 * i + k] = found ? (int32_t)((gk >> (21 * k)) & 0x1FFFFFull) - SE_CLEAR_BIAS : (int32_t)0x80000000;
      }
    }
  }
}
