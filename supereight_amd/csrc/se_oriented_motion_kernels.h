// Batched collision queries for oriented boxes moved along straight segments against the resident map (se_hip_collide_oriented_motions,
// include/se_hip.h): for N motions -- the open box {c + s0 h0 + s1 h1 + s2 h2 : |s_i| < 1} translated by t * d, t in [0, 1], in sub-units of
// 1 / SE_ORIENTED_SUB voxel -- the min over the voxels the moving box touches of classify(Octree::get(v)) (outside the volume: unseen), and
// the exact parameter at which it first touches a blocking voxel.  The host restatement and the literal definition are
// include/se/oriented_motion.hpp.
//
// The geometry is exact integer arithmetic in doubled sub-units, in the two forms of the header.
//   - Touched.  The swept set is the open zonotope with generators h0, h1, h2, d / 2 about c + d / 2; a cube (corner v, side s in voxels) is
//     touched iff none of the 21 axes e_k, g_i x g_j, g_i x e_k (g = h0, h1, h2, d) separates:
//         |a . (32 v + 16 s - 2 c - d)| >= 2 sum_i |a . h_i| + |a . d| + 16 s sum_k |a_k|.
//     This is the set of cubes the interval form calls touched: the union of the open boxes B(t) over [0, 1] is that zonotope (the ends add
//     nothing: an open set that B(0) meets, B(eps) meets too), and for two open convex polytopes the axes above decide.  int64 throughout:
//     |a_k| <= 2^29 for the fifteen axes without d and <= 2^33 for the six with it, both sides below 2^59.
//   - Entry parameter.  Over the fifteen axes of the static query, with p = a . (32 v + 16 s - 2 c), q = 2 a . d, R = 2 sum_i |a . h_i| +
//     16 s sum_k |a_k|: t_in = max(0, max over the axes with q != 0 of (p sign(q) - R) / |q|).  |p| < 2^53, |q| < 2^50, R < 2^49: the
//     numerators stay below 2^54, and two such rationals are compared by cross-multiplication in __int128.  Only a touched cube's t_in is
//     ever asked for, so the upper ends of the intervals are not formed.  Nothing is divided or rounded before the final conversion.
// Per axis the query keeps a (int64 x 3), S = sum_k |a_k|, K = -2 a . c, R = 2 sum_i |a . h_i| (2^62 for a zero axis: it never separates) and
// Q = 2 a . d; p is then K + 32 a . v + 16 s (a_x + a_y + a_z), affine in the cube's position, and the left side above is p - Q / 2.  The six
// axes with d are orthogonal to d: their Q is 0 and they take no part in the entry parameter.
// The entry parameter of a part of a cube is never smaller than the cube's, so skipping an octant whose entry parameter is not below the best
// found so far loses nothing.
//
// One wave64 per motion (grid-stride over int64 n), wave-uniform control flow, on the frontier descent of se_frontier.h; the frontier holds
// the present touched octants that can still change an output.
//   - the 21 axes of a query are wave-uniform: lane k computes axis k once per query into LDS (SeOrientedMotionAxes, beside the frontier), and
//     every test reads them from there at a uniform address;
//   - an octant step: each lane tests its child; an absent touched child folds classify(value_[child]) into the status and, if that class
//     blocks, its entry parameter into the lane's best (exact: every voxel of the octant reads that value); present touched children are pushed;
//   - at a block the lanes are its 8 x 8 columns: per axis a lane forms the x / y part of p once and steps z by 32 a_z; the first three axes are
//     the sweep's bounding interval per axis, and a block none of whose columns survives them skips the other eighteen; the loads of the
//     touched voxels are issued after all the tests (unrolled, in flight together); the entry parameter is formed for the touched voxels that
//     block only;
//   - each lane keeps its best (num, den) as int64; the wave minimum is taken after a step in which some lane improved;
//   - an octant or block is skipped iff it can change neither output: the status is already occupied and the t outputs are not wanted or the
//     octant's entry parameter is not below the best.  Without t outputs the search stops at the first occupied step;
//   - lane 0 reduces the best pair by its gcd and converts it, once per motion.
// Every loop is bounded by the structure: the descent by the argument in se_frontier.h, whatever the test; a leaf step visits at most 64
// blocks; the axis loops run 21 or 15 times and the column loops 8; Euclid's gcd replaces (a, b) by (b, a mod b) with a mod b < b, so b
// reaches 0 after at most 2 * 54 steps for terms below 2^54.  No array is indexed by a lane-dependent value.
#pragma once
#include "se_oriented_kernels.h"

#define SE_ORIENTED_MOVE_LIMIT (1 << 18)    // |d_k| <= 2^18 sub-units
#define SE_ORIENTED_MOTION_AXES 21
#define SE_ORIENTED_ENTRY_AXES 15           // the axes without d come first: those of the static query, in its order

struct OrientedMotionArgs {
  const int32_t* motions; long long n; uint8_t* status; float* t_first; long long* t_exact; float thr; int above; uint32_t stop_at;
};

// The axes of the current query and their constants (LDS; written by lanes 0..20, read by all at uniform addresses).
struct SeOrientedMotionAxes {
  long long ax[24], ay[24], az[24];
  long long sa[24];    // S = |a_x| + |a_y| + |a_z|
  long long k[24];     // K = -2 a . c
  long long r[24];     // R = 2 sum_i |a . h_i|, SE_ORIENTED_NEVER for a zero axis
  long long q[24];     // Q = 2 a . d (0 for the axes with d)
};

// an / ad < bn / bd (denominators positive; terms below 2^54)
__device__ __forceinline__ bool se_rat_less_wide(long long an, long long ad, long long bn, long long bd) {
  return (__int128)an * bd < (__int128)bn * ad;
}

__device__ __forceinline__ long long se_readlane64(long long v, int w) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, w);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((unsigned long long)v >> 32), w);
  return (long long)(((unsigned long long)hi << 32) | lo);
}

// Lane k < 21 computes axis k of the motion (c, h[i], d) into q.  Axis k = u x w: e_k for k < 3, then h1 x h2, h2 x h0, h0 x h1, then h_i x e_j
// at 6 + 3 i + j, then h_i x d at 15 + i, then d x e_j at 18 + j.  (The selects are on the lane id: c, h and d stay in scalar registers.)
__device__ __forceinline__ void se_oriented_motion_axes(SeOrientedMotionAxes& q, const int* c, const int (*h)[3], const int* d) {
  const int lane = (int)(threadIdx.x & 63u);
  if (lane >= SE_ORIENTED_MOTION_AXES) return;
  // u, w: 0..2 a half-axis, 3 the displacement, 4..6 a unit vector
  int iu, iw;
  if (lane < 3) { iu = 4 + (lane + 1) % 3; iw = 4 + (lane + 2) % 3; }
  else if (lane < 6) { iu = (lane - 2) % 3; iw = (lane - 1) % 3; }
  else if (lane < 15) { iu = (lane - 6) / 3; iw = 4 + (lane - 6) % 3; }
  else if (lane < 18) { iu = lane - 15; iw = 3; }
  else { iu = 3; iw = 4 + (lane - 18); }
  long long u[3], w[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    u[k] = iu == 0 ? h[0][k] : (iu == 1 ? h[1][k] : (iu == 2 ? h[2][k] : (iu == 3 ? d[k] : (iu - 4 == k ? 1 : 0))));
    w[k] = iw == 0 ? h[0][k] : (iw == 1 ? h[1][k] : (iw == 2 ? h[2][k] : (iw == 3 ? d[k] : (iw - 4 == k ? 1 : 0))));
  }
  const long long a[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
  long long r = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i) r += se_abs64(a[0] * h[i][0] + a[1] * h[i][1] + a[2] * h[i][2]);
  const bool zero = a[0] == 0 && a[1] == 0 && a[2] == 0;
  q.ax[lane] = a[0]; q.ay[lane] = a[1]; q.az[lane] = a[2];
  q.sa[lane] = se_abs64(a[0]) + se_abs64(a[1]) + se_abs64(a[2]);
  q.k[lane] = -2 * (a[0] * c[0] + a[1] * c[1] + a[2] * c[2]);
  q.r[lane] = zero ? SE_ORIENTED_NEVER : 2 * r;
  q.q[lane] = lane < SE_ORIENTED_ENTRY_AXES ? 2 * (a[0] * d[0] + a[1] * d[1] + a[2] * d[2]) : 0;   // (a x d) . d = 0
}

// The exact test of the cube (corner x, y, z; side s, in voxels): true iff none of the 21 axes separates it from the sweep.
__device__ __forceinline__ bool se_oriented_motion_touched(const SeOrientedMotionAxes& q, int x, int y, int z, int s) {
  bool touched = true;
  for (int k = 0; k < SE_ORIENTED_MOTION_AXES; ++k) {
    const long long ax = q.ax[k], ay = q.ay[k], az = q.az[k], hq = q.q[k] >> 1;   // (Q is even)
    const long long lhs = q.k[k] + 32 * (ax * x + ay * y + az * z) + 16ll * s * (ax + ay + az) - hq;
    touched = touched && se_abs64(lhs) < q.r[k] + se_abs64(hq) + 16ll * s * q.sa[k];
  }
  return touched;
}

// The entry parameter tn / td of a touched cube (corner x, y, z; side s, in voxels): the largest of 0 and the lower ends over the axes that move.
__device__ __forceinline__ void se_oriented_motion_entry(const SeOrientedMotionAxes& q, int x, int y, int z, int s, long long& tn, long long& td) {
  tn = 0; td = 1;
  for (int k = 0; k < SE_ORIENTED_ENTRY_AXES; ++k) {
    const long long Q = q.q[k];
    if (Q == 0) continue;   // (uniform)
    const long long ax = q.ax[k], ay = q.ay[k], az = q.az[k];
    const long long p = q.k[k] + 32 * (ax * x + ay * y + az * z) + 16ll * s * (ax + ay + az);
    const long long ln = (Q > 0 ? p : -p) - (q.r[k] + 16ll * s * q.sa[k]), ld = se_abs64(Q);
    if (ln > 0 && se_rat_less_wide(tn, td, ln, ld)) { tn = ln; td = ld; }
  }
}

// If some lane improved its best bn / bd: the wave's smallest pair into every lane's best and into the uniform gn / gd.
__device__ __forceinline__ void se_oriented_motion_settle(long long& bn, long long& bd, bool& improved, long long& gn, long long& gd) {
  if (__ballot(improved) == 0ull) return;
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    const long long on = __shfl_xor(bn, off), od = __shfl_xor(bd, off);
    if (se_rat_less_wide(on, od, bn, bd)) { bn = on; bd = od; }
  }
  gn = bn = se_readlane64(bn, 0);   // (equal values may be written differently: every lane takes lane 0's pair)
  gd = bd = se_readlane64(bd, 0);
  improved = false;
}

// The voxels of the block at slot `slot` (corner bc) that the motion touches: their classes folded from empty (returned as the wave's min),
// and the entry parameter of those that block folded into the lane's best bn / bd.  Lane = column (x, y) of the block; bit z of `sep`: some
// axis separates voxel z of the column from the sweep.
__device__ __forceinline__ uint32_t se_oriented_motion_block(const DevMap& m, const FieldConst fc, float thr, int above, uint32_t stop_at, bool want_t, uint32_t slot,
                                                             int bcx, int bcy, int bcz, const SeOrientedMotionAxes& q, long long& bn, long long& bd, bool& improved) {
  const int lane = (int)(threadIdx.x & 63u);
  const int x = bcx + (lane & 7), y = bcy + (lane >> 3);
  uint32_t sep = 0u;
  for (int k = 0; k < SE_ORIENTED_MOTION_AXES; ++k) {
    if (k == 3 && __ballot(sep != 0xFFu) == 0ull) break;   // the sweep's bounding interval per axis misses every column
    const long long ax = q.ax[k], ay = q.ay[k], az = q.az[k], hq = q.q[k] >> 1;
    long long lhs = q.k[k] + 32 * (ax * x + ay * y + az * bcz) + 16 * (ax + ay + az) - hq;
    const long long rhs = q.r[k] + se_abs64(hq) + 16 * q.sa[k];
#pragma unroll
    for (int z = 0; z < 8; ++z) {
      if (se_abs64(lhs) >= rhs) sep |= 1u << z;
      lhs += 32 * az;
    }
  }
  float vx[8], vy[8];
#pragma unroll
  for (int z = 0; z < 8; ++z) {
    vx[z] = fc.init_x; vy[z] = fc.init_y;
    if (!(sep & (1u << z))) {
      const size_t vi = se_brick_voxel(slot, z);
      vx[z] = m.vx[vi]; vy[z] = se_ld_y(m, vi);
    }
  }
  uint32_t c = SE_COLLIDE_EMPTY, blocks = 0u;
#pragma unroll
  for (int z = 0; z < 8; ++z)
    if (!(sep & (1u << z))) {
      const uint32_t cls = se_collide_class(vx[z], vy[z], fc, thr, above);
      c = min(c, cls);
      if (cls <= stop_at) blocks |= 1u << z;
    }
  if (want_t) {
    for (int z = 0; z < 8; ++z) {
      const bool need = (blocks >> z) & 1u;
      if (__ballot(need) == 0ull) continue;
      long long tn, td;
      se_oriented_motion_entry(q, x, y, bcz + z, 1, tn, td);
      if (need && se_rat_less_wide(tn, td, bn, bd)) { bn = tn; bd = td; improved = true; }
    }
  }
  return se_collide_wave_min(c);
}

template <bool DENSE>
__global__ __launch_bounds__(SE_WG_COLLIDE) void k_collide_oriented_motions(DevMap m, OrientedMotionArgs a) {
  __shared__ SeFrontier f;
  __shared__ SeOrientedMotionAxes q;
  const FieldConst fc = se_field_const(m);
  const int lane = (int)(threadIdx.x & 63u);
  se_frontier_init(f, m);
  const int leaf = m.leaf_level;
  const float thr = a.thr;
  const int above = a.above;
  const uint32_t stop_at = a.stop_at;
  const bool want_t = a.t_first != nullptr || a.t_exact != nullptr;

  for (long long i = blockIdx.x; i < a.n; i += gridDim.x) {
    const int32_t* mo = a.motions + 15 * i;
    const int c[3] = {mo[0], mo[1], mo[2]};
    const int h[3][3] = {{mo[3], mo[4], mo[5]}, {mo[6], mo[7], mo[8]}, {mo[9], mo[10], mo[11]}};
    const int d[3] = {mo[12], mo[13], mo[14]};
    bool valid = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const long long e = (long long)c[k] + d[k];
      valid = valid && c[k] >= -SE_ORIENTED_C_LIMIT && c[k] <= SE_ORIENTED_C_LIMIT && d[k] >= -SE_ORIENTED_MOVE_LIMIT && d[k] <= SE_ORIENTED_MOVE_LIMIT &&
              e >= -SE_ORIENTED_C_LIMIT && e <= SE_ORIENTED_C_LIMIT;
#pragma unroll
      for (int j = 0; j < 3; ++j) valid = valid && h[j][k] >= -SE_ORIENTED_H_LIMIT && h[j][k] <= SE_ORIENTED_H_LIMIT;
    }
    if (valid) {   // (within the bounds: every term below 2^43)
      const long long det = (long long)h[0][0] * ((long long)h[1][1] * h[2][2] - (long long)h[1][2] * h[2][1]) +
                            (long long)h[0][1] * ((long long)h[1][2] * h[2][0] - (long long)h[1][0] * h[2][2]) +
                            (long long)h[0][2] * ((long long)h[1][0] * h[2][1] - (long long)h[1][1] * h[2][0]);
      valid = det != 0;
    }
    uint32_t st = valid ? SE_COLLIDE_EMPTY : SE_COLLIDE_INVALID;
    bool run = valid;
    long long gn = 2, gd = 1;   // the wave's best entry parameter of a blocking voxel so far (2 / 1: none)
    __syncthreads();   // the last query's reads of q are done
    if (valid) {
      const int lim = SE_ORIENTED_SUB * m.size;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int ext = abs(h[0][k]) + abs(h[1][k]) + abs(h[2][k]);   // at t the box spans (c_k + t d_k - ext, c_k + t d_k + ext), open
        const int lo = c[k] - ext, hi = c[k] + ext;
        const int mn = min(lo, lo + d[k]), mx = max(hi, hi + d[k]);
        if (mn < 0 || mx > lim) st = SE_COLLIDE_UNSEEN;   // a part outside the volume
        if (mx <= 0 || mn >= lim) run = false;            // nothing inside it
        // the voxels outside the volume are unseen; per face, the parameter at which the first of them is touched
        if (stop_at >= SE_COLLIDE_UNSEEN) {
          long long fn = 2, fd = 1;
          if (lo < 0 || hi > lim) { fn = 0; }
          else if (d[k] < 0 && lo < -d[k]) { fn = lo; fd = -d[k]; }
          else if (d[k] > 0 && lim - hi < d[k]) { fn = lim - hi; fd = d[k]; }
          if (se_rat_less_wide(fn, fd, gn, gd)) { gn = fn; gd = fd; }
        }
      }
      se_oriented_motion_axes(q, c, h, d);
    }
    long long bn = gn, bd = gd;    // this lane's best; equal to the wave's after each step
    bool improved = false;
    int l;
    SeFrontierStep t;
    se_frontier_root(f, l);   // (its barriers also publish q)
    while (run && se_frontier_pop(f, m, l, t)) {
      const int s = t.s;
      bool ov = t.live && se_oriented_motion_touched(q, t.cx * s, t.cy * s, t.cz * s, s);
      long long tn = 0, td = 1;
      if (want_t) se_oriented_motion_entry(q, t.cx * s, t.cy * s, t.cz * s, s, tn, td);
      // an octant that can change neither output is dropped
      if (st == SE_COLLIDE_OCC) ov = ov && want_t && se_rat_less_wide(tn, td, gn, gd);
      const uint32_t e = se_frontier_entry(f, m, t, ov);
      const bool present = ov && e != 0u && e != SE_PENDING;
      // absent touched children: the whole octant has the class of value_[child]
      uint32_t cls = SE_COLLIDE_EMPTY;
      if (ov && !present) {
        cls = se_collide_class(m.nx[(size_t)t.nid * 8 + t.c], m.ny[(size_t)t.nid * 8 + t.c], fc, thr, above);
        if (want_t && cls <= stop_at && se_rat_less_wide(tn, td, bn, bd)) { bn = tn; bd = td; improved = true; }
      }
      st = min(st, se_collide_wave_min(cls));
      if (t.L < leaf) {
        se_frontier_push(f, t, present, e, l);
      } else {
        __syncthreads();   // the leaf step's barrier (se_frontier.h)
        unsigned long long b = __ballot(present);
        while (b) {
          const int w = (int)__builtin_ctzll(b);
          b &= b - 1ull;
          if (st == SE_COLLIDE_OCC) {   // the best may have improved since this block passed the test above
            if (!want_t) break;
            if (!se_rat_less_wide(se_readlane64(tn, w), se_readlane64(td, w), gn, gd)) continue;
          }
          int qx, qy, qz;
          const uint32_t slot = se_frontier_block<DENSE>(m, t, e, w, qx, qy, qz);
          st = min(st, se_oriented_motion_block(m, fc, thr, above, stop_at, want_t, slot, qx * 8, qy * 8, qz * 8, q, bn, bd, improved));
          se_oriented_motion_settle(bn, bd, improved, gn, gd);
        }
      }
      se_oriented_motion_settle(bn, bd, improved, gn, gd);
      if (st == SE_COLLIDE_OCC && (!want_t || gn == 0)) break;   // nothing can change either output any more
    }
    if (lane == 0) {
      a.status[i] = (uint8_t)st;
      if (want_t) {
        long long num = valid ? gn : -1, den = valid ? gd : 1;
        long long x = num < 0 ? -num : num, y = den;
        while (y) { const long long r = x % y; x = y; y = r; }   // Euclid: x ends as gcd(num, den) >= 1
        num /= x; den /= x;
        if (a.t_exact) { a.t_exact[2 * i] = num; a.t_exact[2 * i + 1] = den; }
        if (a.t_first) a.t_first[i] = (float)((double)num / (double)den);
      }
    }
  }
}
