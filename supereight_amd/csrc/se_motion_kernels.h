// Batched collision queries for boxes moved along straight segments against the resident map (se_hip_collide_motions, include/se_hip.h): for
// N motions -- the box [lo, lo + side) translated by t * d, t in [0, 1], in whole voxels -- the min over the voxels the moving box touches of
// classify(Octree::get(v)) (outside the volume: unseen), and the parameter t_first at which it first touches a blocking voxel.  The host
// restatement and the literal definition are include/se/motion_collision.hpp.
//
// The geometry is exact integer arithmetic.  A cube (corner c, side s) is touched iff L < U, where L is the largest of 0 and the lower ends
// and U the smallest of 1 and the upper ends of the per-axis open intervals
//     d_k > 0: ((c_k - hi_k) / d_k, (c_k + s - lo_k) / d_k)      d_k < 0: ((lo_k - c_k - s) / |d_k|, (hi_k - c_k) / |d_k|)      hi = lo + side
// (an axis with d_k = 0 gives the static half-open overlap test).  L is the cube's entry parameter.  Rationals are (num, den) pairs of int32
// -- a valid motion has lo, hi, lo + d, hi + d in [-2^20, 2^20] and the cubes tested lie in [0, size], so every term is below 2^22 in
// magnitude -- compared by cross-multiplication in int64 (products below 2^44).  The entry parameter of a part of a cube is never smaller than
// the cube's, so skipping an octant whose entry parameter is not below the best found so far loses nothing.
//
// One wave64 per motion (grid-stride over int64 n), wave-uniform control flow, on the frontier descent of se_frontier.h; the frontier holds
// the present touched octants that can still change an output.
//   - an absent touched child folds classify(value_[child]) into the status and, if that class blocks, its entry parameter into the lane's
//     best: exact, because every voxel of the octant reads that value;
//   - at a block the lanes are its 8 x 8 columns: a lane forms the x / y part of its column's interval once and then tests its 8 z voxels
//     (loads unrolled, in flight together);
//   - each lane keeps its best (num, den); the wave minimum is taken after a step in which some lane improved, and once more is not needed at
//     the end: the uniform best is what pruning reads and what is written;
//   - an octant or block is skipped iff it can change neither output: the status is already occupied and t_first is not wanted or the
//     octant's entry parameter is not below the best.  Without t_first the search stops at the first occupied step, as the box kernel does.
// Every loop is bounded by the structure: the descent by the argument in se_frontier.h, whatever the test, and a leaf step visits at most
// 64 blocks.
#pragma once
#include "se_collide_kernels.h"

#define SE_MOTION_LIMIT (1 << 20)       // lo, lo + side, lo + d, lo + side + d within [-2^20, 2^20], else the motion is invalid

struct MotionArgs { const int32_t* motions; long long n; uint8_t* status; float* t_first; float thr; int above; uint32_t stop_at; };

// an / ad < bn / bd (denominators positive)
__device__ __forceinline__ bool se_rat_less(int an, int ad, int bn, int bd) { return (long long)an * bd < (long long)bn * ad; }

// Axis k of the test of a cube [c, c + s): folds the axis's open interval into L = Ln / Ld (from below) and U = Un / Ud (from above); false iff
// the axis does not move and misses the cube.
__device__ __forceinline__ bool se_motion_axis(int lo, int hi, int d, int c, int s, int& Ln, int& Ld, int& Un, int& Ud) {
  if (d == 0) return lo < c + s && hi > c;
  const int a = d > 0 ? d : -d;
  const int ln = d > 0 ? c - hi : lo - c - s;
  const int un = d > 0 ? c + s - lo : hi - c;
  if (se_rat_less(Ln, Ld, ln, a)) { Ln = ln; Ld = a; }
  if (se_rat_less(un, a, Un, Ud)) { Un = un; Ud = a; }
  return true;
}

// If some lane improved its best bn / bd: the wave's smallest pair into every lane's best and into the uniform gn / gd.
__device__ __forceinline__ void se_motion_settle(int& bn, int& bd, bool& improved, int& gn, int& gd) {
  if (__ballot(improved) == 0ull) return;
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    const int on = __shfl_xor(bn, off), od = __shfl_xor(bd, off);
    if (se_rat_less(on, od, bn, bd)) { bn = on; bd = od; }
  }
  gn = bn = __builtin_amdgcn_readfirstlane(bn);   // (equal values may be written differently: every lane takes lane 0's pair)
  gd = bd = __builtin_amdgcn_readfirstlane(bd);
  improved = false;
}

// The voxels of the block at slot `slot` (corner bc) that the motion touches: their classes folded from empty (returned as the wave's min),
// and the entry parameter of those that block folded into the lane's best bn / bd.  Lane = column (x, y) of the block.
__device__ __forceinline__ uint32_t se_motion_block(const DevMap& m, const FieldConst fc, float thr, int above, uint32_t stop_at, bool want_t, uint32_t slot,
                                                    int bcx, int bcy, int bcz, const int* lo, const int* hi, const int* d, int& bn, int& bd, bool& improved) {
  const int lane = (int)(threadIdx.x & 63u);
  int cLn = 0, cLd = 1, cUn = 1, cUd = 1;
  bool col = se_motion_axis(lo[0], hi[0], d[0], bcx + (lane & 7), 1, cLn, cLd, cUn, cUd);
  col = se_motion_axis(lo[1], hi[1], d[1], bcy + (lane >> 3), 1, cLn, cLd, cUn, cUd) && col;
  bool t[8];
  int zn[8], zd[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    int Un = cUn, Ud = cUd;
    zn[k] = cLn; zd[k] = cLd;
    t[k] = se_motion_axis(lo[2], hi[2], d[2], bcz + k, 1, zn[k], zd[k], Un, Ud) && col;
    t[k] = t[k] && se_rat_less(zn[k], zd[k], Un, Ud);
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
  uint32_t c = SE_COLLIDE_EMPTY;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (t[k]) {
      const uint32_t cls = se_collide_class(vx[k], vy[k], fc, thr, above);
      c = min(c, cls);
      if (want_t && cls <= stop_at && se_rat_less(zn[k], zd[k], bn, bd)) { bn = zn[k]; bd = zd[k]; improved = true; }
    }
  }
  return se_collide_wave_min(c);
}

template <bool DENSE>
__global__ __launch_bounds__(SE_WG_COLLIDE) void k_collide_motions(DevMap m, MotionArgs a) {
  __shared__ SeFrontier f;
  const FieldConst fc = se_field_const(m);
  const int lane = (int)(threadIdx.x & 63u);
  se_frontier_init(f, m);
  const int leaf = m.leaf_level;
  const float thr = a.thr;
  const int above = a.above;
  const uint32_t stop_at = a.stop_at;
  const bool want_t = a.t_first != nullptr;

  for (long long i = blockIdx.x; i < a.n; i += gridDim.x) {
    const int32_t* mo = a.motions + 9 * i;
    int lo[3], hi[3], d[3];
    bool valid = true, run = true;
    uint32_t st = SE_COLLIDE_EMPTY;
    int gn = 2, gd = 1;   // the wave's best entry parameter of a blocking voxel so far (2 / 1: none, SE_HIP_MOTION_FREE)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const long long l0 = mo[k], sd = mo[3 + k], dk = mo[6 + k];
      const long long h0 = l0 + sd, l1 = l0 + dk, h1 = h0 + dk;
      valid = valid && sd >= 1 && l0 >= -SE_MOTION_LIMIT && l0 <= SE_MOTION_LIMIT && h0 >= -SE_MOTION_LIMIT && h0 <= SE_MOTION_LIMIT &&
              l1 >= -SE_MOTION_LIMIT && l1 <= SE_MOTION_LIMIT && h1 >= -SE_MOTION_LIMIT && h1 <= SE_MOTION_LIMIT;
      lo[k] = (int)l0; hi[k] = (int)h0; d[k] = (int)dk;
    }
    if (!valid) { st = SE_COLLIDE_INVALID; run = false; }
    if (valid) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int mn = min(lo[k], lo[k] + d[k]), mx = max(hi[k], hi[k] + d[k]);   // the bounding box of the motion
        if (max(mn, 0) >= min(mx, m.size)) run = false;                            // nothing inside the volume
        // the voxels outside the volume are unseen; per face, the parameter at which the first of them is touched
        if (mn < 0 || mx > m.size) st = SE_COLLIDE_UNSEEN;
        if (stop_at >= SE_COLLIDE_UNSEEN) {
          int fn = 2, fd = 1;
          if (lo[k] < 0 || hi[k] > m.size) { fn = 0; }
          else if (d[k] < 0 && lo[k] < -d[k]) { fn = lo[k]; fd = -d[k]; }
          else if (d[k] > 0 && m.size - hi[k] < d[k]) { fn = m.size - hi[k]; fd = d[k]; }
          if (se_rat_less(fn, fd, gn, gd)) { gn = fn; gd = fd; }
        }
      }
    }
    int bn = gn, bd = gd;    // this lane's best; equal to the wave's after each step
    bool improved = false;
    int l;
    SeFrontierStep t;
    se_frontier_root(f, l);
    while (run && se_frontier_pop(f, m, l, t)) {
      const int s = t.s, cx = t.cx, cy = t.cy, cz = t.cz;
      const uint32_t e = se_frontier_entry(f, m, t, t.live);
      const bool present = t.live && e != 0u && e != SE_PENDING;
      // the exact test of the child octant; tn / td its entry parameter
      int tn = 0, td = 1, Un = 1, Ud = 1;
      bool ov = se_motion_axis(lo[0], hi[0], d[0], cx * s, s, tn, td, Un, Ud);
      ov = se_motion_axis(lo[1], hi[1], d[1], cy * s, s, tn, td, Un, Ud) && ov;
      ov = se_motion_axis(lo[2], hi[2], d[2], cz * s, s, tn, td, Un, Ud) && ov;
      ov = ov && t.live && se_rat_less(tn, td, Un, Ud);
      // an octant that can change neither output is dropped
      if (st == SE_COLLIDE_OCC) ov = ov && want_t && se_rat_less(tn, td, gn, gd);
      // absent touched children: the whole octant has the class of value_[child]
      const bool absent = ov && !present;
      uint32_t cls = SE_COLLIDE_EMPTY;
      if (absent) {
        cls = se_collide_class(m.nx[(size_t)t.nid * 8 + t.c], m.ny[(size_t)t.nid * 8 + t.c], fc, thr, above);
        if (want_t && cls <= stop_at && se_rat_less(tn, td, bn, bd)) { bn = tn; bd = td; improved = true; }
      }
      st = min(st, se_collide_wave_min(cls));
      const bool hit = ov && present;
      if (t.L < leaf) {
        se_frontier_push(f, t, hit, e, l);
      } else {
        __syncthreads();   // the leaf step's barrier (se_frontier.h)
        unsigned long long b = __ballot(hit);
        while (b) {
          const int w = (int)__builtin_ctzll(b);
          b &= b - 1ull;
          if (st == SE_COLLIDE_OCC) {   // the best may have improved since this block passed the test above
            if (!want_t) break;
            const int wn = __builtin_amdgcn_readlane(tn, w), wd = __builtin_amdgcn_readlane(td, w);
            if (!se_rat_less(wn, wd, gn, gd)) continue;
          }
          int qx, qy, qz;
          const uint32_t slot = se_frontier_block<DENSE>(m, t, e, w, qx, qy, qz);
          st = min(st, se_motion_block(m, fc, thr, above, stop_at, want_t, slot, qx * 8, qy * 8, qz * 8, lo, hi, d, bn, bd, improved));
          se_motion_settle(bn, bd, improved, gn, gd);
        }
      }
      se_motion_settle(bn, bd, improved, gn, gd);
      if (st == SE_COLLIDE_OCC && (!want_t || gn == 0)) break;   // nothing can change either output any more
    }
    if (lane == 0) {
      a.status[i] = (uint8_t)st;
      if (want_t) a.t_first[i] = valid ? (float)gn / (float)gd : -1.0f;
    }
  }
}
