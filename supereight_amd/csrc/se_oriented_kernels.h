// Batched collision queries for oriented boxes against the resident map (se_hip_collide_oriented, include/se_hip.h): for N boxes -- centre c
// and three half-axes h0, h1, h2 in sub-units of 1 / SE_ORIENTED_SUB voxel, the open set {c + s0 h0 + s1 h1 + s2 h2 : |s_i| < 1} -- the min
// over the voxels the box touches of classify(Octree::get(v)) (outside the volume: unseen).  The host restatement and the literal definition
// are include/se/oriented_collision.hpp.
//
// The geometry is exact integer arithmetic: a separating-axis test in doubled sub-units.  For a cube (corner v, side s in voxels) the doubled
// offset from the box centre to the cube centre is m = 32 v + 16 s - 2 c and the doubled half-side e = 16 s; an axis a != 0 separates iff
//     |a . m| >= 2 sum_i |a . h_i| + e sum_k |a_k|
// and the cube is touched iff none of the 15 axes e_k, h_i x h_j, h_i x e_k separates.  With |c_k| <= 2^20 and |h_ik| <= 2^14 (else the box is
// invalid) and sizes up to 8192: |a_k| <= 2^29 (int32), |m_k| < 2^22, |a . m| < 2^53, the right-hand side < 2^49 -- int64 throughout, nothing is
// rounded.  Per axis the query keeps a (int32 x 3), K = -2 a . c, R = 2 sum_i |a . h_i| and S = sum_k |a_k|; the left side is then
// K + 32 a . v + 16 s (a_x + a_y + a_z), affine in the cube's position.  A zero axis (a half-axis parallel to a cube edge) gets R = 2^62:
// it never separates, as the definition asks.
//
// One wave64 per box (grid-stride over int64 n), wave-uniform control flow, on the frontier descent of se_frontier.h; the frontier holds
// the present touched octants.
//   - the 15 axes of a query are wave-uniform: lane k computes axis k once per query into LDS (SeOrientedAxes, beside the frontier), and
//     every test reads them from there at a uniform address -- no lane keeps a copy in its registers across steps;
//   - an octant step: each lane tests its child with the predicate; an absent touched child folds classify(value_[child]) (exact: an open
//     set that meets an open cube meets the open cube of one of its voxels, and every voxel of the octant reads that value);
//   - at a block the lanes are its 8 x 8 columns: per axis a lane forms the x / y part of the left side once and steps z by 32 a_z; the
//     first three axes are the box's bounding interval per axis, and a block none of whose columns survives them skips the other twelve;
//     the loads of the touched voxels are issued after all the tests (unrolled, in flight together);
//   - the search stops at the first occupied step, as the box kernel does.
// Every loop is bounded by the structure: the descent by the argument in se_frontier.h, whatever the test; a leaf step visits at most
// 64 blocks; the axis loops run 15 times and the column loops 8.  No array is indexed by a lane-dependent value: there is no scratch.
#pragma once
#include "se_collide_kernels.h"

#define SE_ORIENTED_SUB 16                  // sub-units per voxel
#define SE_ORIENTED_C_LIMIT (1 << 20)       // |c_k| <= 2^20 sub-units
#define SE_ORIENTED_H_LIMIT (1 << 14)       // |h_ik| <= 2^14 sub-units
#define SE_ORIENTED_AXES 15
#define SE_ORIENTED_NEVER (1ll << 62)       // R of a zero axis

struct OrientedArgs { const int32_t* boxes; long long n; uint8_t* status; float thr; int above; };

// The axes of the current query and their constants (LDS; written by lanes 0..14, read by all at uniform addresses).
struct SeOrientedAxes {
  int ax[16], ay[16], az[16];
  int sa[16];          // S = |a_x| + |a_y| + |a_z| (at most 3 * 2^29)
  long long k[16];     // K = -2 a . c
  long long r[16];     // R = 2 sum_i |a . h_i|, SE_ORIENTED_NEVER for a zero axis
};

__device__ __forceinline__ long long se_abs64(long long v) { return v < 0 ? -v : v; }

// Lane k < 15 computes axis k of the box (c, h[i]) into q.  Axis k = u x w: e_k = e_(k+1) x e_(k+2) for k < 3, then h1 x h2, h2 x h0, h0 x h1,
// then h_i x e_j at 6 + 3 i + j.  (The selects are on the lane id: c and h stay in scalar registers.)
__device__ __forceinline__ void se_oriented_axes(SeOrientedAxes& q, const int* c, const int (*h)[3]) {
  const int lane = (int)(threadIdx.x & 63u);
  if (lane >= SE_ORIENTED_AXES) return;
  const int iu = lane < 3 ? -1 : (lane < 6 ? (lane - 2) % 3 : (lane - 6) / 3);   // u = h_iu (or a unit vector)
  const int iw = lane < 6 ? (lane < 3 ? -1 : (lane - 1) % 3) : -1;               // w = h_iw (or a unit vector)
  const int eu = lane < 3 ? (lane + 1) % 3 : -1;                                 // u = e_eu
  const int ew = lane < 3 ? (lane + 2) % 3 : (lane >= 6 ? (lane - 6) % 3 : -1);  // w = e_ew
  long long u[3], w[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    u[k] = iu == 0 ? h[0][k] : (iu == 1 ? h[1][k] : (iu == 2 ? h[2][k] : (eu == k ? 1 : 0)));
    w[k] = iw == 0 ? h[0][k] : (iw == 1 ? h[1][k] : (iw == 2 ? h[2][k] : (ew == k ? 1 : 0)));
  }
  const long long a[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
  long long r = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i) r += se_abs64(a[0] * h[i][0] + a[1] * h[i][1] + a[2] * h[i][2]);
  const bool zero = a[0] == 0 && a[1] == 0 && a[2] == 0;
  q.ax[lane] = (int)a[0]; q.ay[lane] = (int)a[1]; q.az[lane] = (int)a[2];
  q.sa[lane] = (int)(se_abs64(a[0]) + se_abs64(a[1]) + se_abs64(a[2]));
  q.k[lane] = -2 * (a[0] * c[0] + a[1] * c[1] + a[2] * c[2]);
  q.r[lane] = zero ? SE_ORIENTED_NEVER : 2 * r;
}

// The exact test of the cube (corner x, y, z; side s, in voxels): true iff no axis separates it from the box.
__device__ __forceinline__ bool se_oriented_touched(const SeOrientedAxes& q, int x, int y, int z, int s) {
  bool touched = true;
  for (int k = 0; k < SE_ORIENTED_AXES; ++k) {
    const long long ax = q.ax[k], ay = q.ay[k], az = q.az[k];
    const long long lhs = q.k[k] + 32 * (ax * x + ay * y + az * z) + 16ll * s * (ax + ay + az);
    touched = touched && se_abs64(lhs) < q.r[k] + 16ll * s * q.sa[k];
  }
  return touched;
}

// The voxels of the block at slot `slot` (corner bc) that the box touches, their classes folded from empty (returned as the wave's min).
// Lane = column (x, y) of the block; bit z of `sep`: some axis separates voxel z of the column from the box.
__device__ __forceinline__ uint32_t se_oriented_block(const DevMap& m, const FieldConst fc, float thr, int above, uint32_t slot, int bcx, int bcy, int bcz,
                                                      const SeOrientedAxes& q) {
  const int lane = (int)(threadIdx.x & 63u);
  const int x = bcx + (lane & 7), y = bcy + (lane >> 3);
  uint32_t sep = 0u;
  for (int k = 0; k < SE_ORIENTED_AXES; ++k) {
    if (k == 3 && __ballot(sep != 0xFFu) == 0ull) break;   // the box's bounding interval per axis misses every column
    const long long ax = q.ax[k], ay = q.ay[k], az = q.az[k];
    long long lhs = q.k[k] + 32 * (ax * x + ay * y + az * bcz) + 16 * (ax + ay + az);
    const long long rhs = q.r[k] + 16ll * q.sa[k];
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
  uint32_t c = SE_COLLIDE_EMPTY;
#pragma unroll
  for (int z = 0; z < 8; ++z)
    if (!(sep & (1u << z))) c = min(c, se_collide_class(vx[z], vy[z], fc, thr, above));
  return se_collide_wave_min(c);
}

template <bool DENSE>
__global__ __launch_bounds__(SE_WG_COLLIDE) void k_collide_oriented(DevMap m, OrientedArgs a) {
  __shared__ SeFrontier f;
  __shared__ SeOrientedAxes q;
  const FieldConst fc = se_field_const(m);
  const int lane = (int)(threadIdx.x & 63u);
  se_frontier_init(f, m);
  const int leaf = m.leaf_level;
  const float thr = a.thr;
  const int above = a.above;

  for (long long i = blockIdx.x; i < a.n; i += gridDim.x) {
    const int32_t* bx = a.boxes + 12 * i;
    const int c[3] = {bx[0], bx[1], bx[2]};
    const int h[3][3] = {{bx[3], bx[4], bx[5]}, {bx[6], bx[7], bx[8]}, {bx[9], bx[10], bx[11]}};
    bool valid = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      valid = valid && c[k] >= -SE_ORIENTED_C_LIMIT && c[k] <= SE_ORIENTED_C_LIMIT;
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
    __syncthreads();   // the last query's reads of q are done
    if (valid) {
      const int lim = SE_ORIENTED_SUB * m.size;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int ext = abs(h[0][k]) + abs(h[1][k]) + abs(h[2][k]);   // the box spans (c_k - ext, c_k + ext), open
        if (c[k] - ext < 0 || c[k] + ext > lim) st = SE_COLLIDE_UNSEEN;   // a part outside the volume
        if (c[k] + ext <= 0 || c[k] - ext >= lim) run = false;            // nothing inside it
      }
      se_oriented_axes(q, c, h);
    }
    int l;
    SeFrontierStep t;
    se_frontier_root(f, l);   // (its barriers also publish q)
    while (run && se_frontier_pop(f, m, l, t)) {
      const int s = t.s;
      const bool ov = t.live && se_oriented_touched(q, t.cx * s, t.cy * s, t.cz * s, s);
      const uint32_t e = se_frontier_entry(f, m, t, ov);
      const bool present = ov && e != 0u && e != SE_PENDING;
      // absent touched children: the whole octant has the class of value_[child]
      uint32_t cls = SE_COLLIDE_EMPTY;
      if (ov && !present) cls = se_collide_class(m.nx[(size_t)t.nid * 8 + t.c], m.ny[(size_t)t.nid * 8 + t.c], fc, thr, above);
      st = min(st, se_collide_wave_min(cls));
      if (t.L < leaf) {
        se_frontier_push(f, t, present, e, l);
      } else {
        __syncthreads();   // the leaf step's barrier (se_frontier.h)
        unsigned long long b = __ballot(present);
        while (b && st != SE_COLLIDE_OCC) {
          const int w = (int)__builtin_ctzll(b);
          b &= b - 1ull;
          int qx, qy, qz;
          const uint32_t slot = se_frontier_block<DENSE>(m, t, e, w, qx, qy, qz);
          st = min(st, se_oriented_block(m, fc, thr, above, slot, qx * 8, qy * 8, qz * 8, q));
        }
      }
      if (st == SE_COLLIDE_OCC) break;   // nothing beats occupied
    }
    if (lane == 0) a.status[i] = (uint8_t)st;
  }
}
