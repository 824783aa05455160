// Exact segment traces of the resident map (se_hip_trace_segments, include/se_hip.h): for N segments a -> b in sub-units of 1 / 16 voxel,
// the voxels the segment touches in the order it touches them, classified as se_hip_collide_boxes classifies them in strict mode -- up to the
// first voxel that blocks: the min class on the way, the entry parameter and the coordinates of the blocking voxel, and how many unseen and
// empty voxels inside the volume precede it.  The host restatement and the literal definition are include/se/segment_trace.hpp.
//
// The geometry is exact integer arithmetic.  With d = b - a, the voxel v is touched iff some t in [0, 1] has 16 v_k < a_k + t d_k < 16 (v_k + 1)
// on every axis: se_hip_collide_motions' rule for a box of side 0.  A valid segment has every coordinate in [-2^22, 2^22], so |d_k| <= 2^23,
// every numerator below 2^24, every cross product below 2^47 and every position numerator a_j den + num d_j below 2^47.
//
// The query is ordered, so it does not use the frontier descent: one lane per segment (grid-stride over int64 n), no LDS, a three-axis integer
// DDA.  A lane keeps the current voxel v, its entry parameter cn / cd and per axis the numerator nn_k of the parameter nn_k / |d_k| at which the
// segment crosses the next grid plane of that axis.  A step takes the smallest of the three by cross-multiplication, advances every axis tied
// at it (through an edge or a corner two or three move at once: the voxels that share only that edge are not touched) and stops when that
// parameter is >= 1.
//   - The index pyramid is read only when v leaves the cached octant: a present block (corner, brick slot) or an absent octant (corner, side
//     8 << sh, the class of value_[child] of the deepest existing node: absent_value_slot, whose sh is the octant's side in blocks).
//   - Inside a block a step reads one voxel; inside an absent octant it reads nothing.
//   - The stretch outside the volume is never stepped: the lane jumps to the volume's entry parameter (the cube test on [0, size)^3) and lands
//     in the voxel that holds P(t + eps) -- per axis floor of the exact position, and where that is a grid plane, the voxel above it for
//     d_j > 0 and the one below for d_j < 0.  After the segment has left the volume nothing more is read: it folds unseen and, under stop_at
//     unseen, blocks there.
//   - COUNT == false (counts not wanted): a non-blocking absent octant is left the same way, by a jump to its exit parameter.  COUNT == true
//     steps through it and counts.
// The walk is bounded by the structure: a step moves at least one axis by one voxel away from the start and the walk ends once the voxel is
// outside the volume, so at most 3 size + 2 steps plus two jumps; the loop counts them down.
#pragma once
#include "se_motion_kernels.h"

#define SE_WG_TRACE 64                  // one wave per workgroup: lanes that finish early idle only until their wave's longest segment ends
#define SE_TRACE_SUB_SHIFT 4            // 16 sub-units per voxel (SE_HIP_ORIENTED_SUB)
#define SE_TRACE_LIMIT (1 << 22)        // every coordinate of a and b within [-2^22, 2^22], else the segment is invalid
#define SE_TRACE_NEVER (1 << 30)        // the crossing numerator of an axis that does not move (over 1: never below 1)
#define SE_TRACE_PRESENT 3u             // cached octant: a present block (else the class of the absent octant)

struct TraceArgs { const int32_t* segments; long long n; uint8_t* status; float* t_first; int32_t* first; int32_t* counts; float thr; int above; uint32_t stop_at; };

// floor((a den + num d) / (16 den)) for d == 0 or where that position is no grid plane; on a grid plane the voxel entered: the one above for
// d > 0, the one below for d < 0.  The quotient lies within +-2^19; a float estimate of it is off by less than one, and the remainder corrects it.
__device__ __forceinline__ int se_trace_land(int a, int d, int num, int den) {
  if (d == 0) return a >> SE_TRACE_SUB_SHIFT;
  const long long P = (long long)a * den + (long long)num * d, Q = (long long)den << SE_TRACE_SUB_SHIFT;
  int q = (int)floorf((float)P / (float)Q);
  long long r = P - (long long)q * Q;
  if (r < 0) { --q; r += Q; }
  if (r >= Q) { ++q; r -= Q; }
  return (r == 0 && d < 0) ? q - 1 : q;
}

// The numerator of the parameter at which axis (a, d) leaves voxel v (over |d|).
__device__ __forceinline__ int se_trace_next(int a, int d, int v) {
  if (d == 0) return SE_TRACE_NEVER;
  return d > 0 ? ((v + 1) << SE_TRACE_SUB_SHIFT) - a : a - (v << SE_TRACE_SUB_SHIFT);
}

// The cube test is se_motion_axis (se_motion_kernels.h) for a box of side 0 -- lo = hi = a -- against the cube in sub-units.
template <bool DENSE, bool COUNT>
__global__ __launch_bounds__(SE_WG_TRACE) void k_trace_segments(DevMap m, TraceArgs a) {
  const FieldConst fc = se_field_const(m);
  const float thr = a.thr;
  const int above = a.above;
  const uint32_t stop_at = a.stop_at;
  const int size = m.size, S = m.size << SE_TRACE_SUB_SHIFT;   // the volume in voxels and in sub-units
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
    const int32_t* sg = a.segments + 6 * i;
    const int ax = sg[0], ay = sg[1], az = sg[2], bx = sg[3], by = sg[4], bz = sg[5];
    const bool valid = ax >= -SE_TRACE_LIMIT && ax <= SE_TRACE_LIMIT && ay >= -SE_TRACE_LIMIT && ay <= SE_TRACE_LIMIT && az >= -SE_TRACE_LIMIT && az <= SE_TRACE_LIMIT &&
                       bx >= -SE_TRACE_LIMIT && bx <= SE_TRACE_LIMIT && by >= -SE_TRACE_LIMIT && by <= SE_TRACE_LIMIT && bz >= -SE_TRACE_LIMIT && bz <= SE_TRACE_LIMIT;
    uint32_t st = valid ? SE_COLLIDE_EMPTY : SE_COLLIDE_INVALID;
    int tn = valid ? 2 : -1, td = 1;                 // t_first: 2 / 1 = nothing blocks (SE_HIP_MOTION_FREE)
    int fx = INT32_MIN, fy = INT32_MIN, fz = INT32_MIN;
    int cu = valid ? 0 : -1, ce = cu;
    const int dx = valid ? bx - ax : 0, dy = valid ? by - ay : 0, dz = valid ? bz - az : 0;
    // a segment in a grid plane touches nothing
    const bool degenerate = (dx == 0 && (ax & 15) == 0) || (dy == 0 && (ay & 15) == 0) || (dz == 0 && (az & 15) == 0);
    if (valid && !degenerate) {
      const int adx = dx == 0 ? 1 : abs(dx), ady = dy == 0 ? 1 : abs(dy), adz = dz == 0 ? 1 : abs(dz);
      const int sx = dx > 0 ? 1 : -1, sy = dy > 0 ? 1 : -1, sz = dz > 0 ? 1 : -1;
      int cn = 0, cd = 1;                            // the entry parameter of the current voxel
      int vx = se_trace_land(ax, dx, 0, 1), vy = se_trace_land(ay, dy, 0, 1), vz = se_trace_land(az, dz, 0, 1);
      int nx = se_trace_next(ax, dx, vx), ny = se_trace_next(ay, dy, vy), nz = se_trace_next(az, dz, vz);
      bool entered = false;                          // the walk has been inside the volume
      int osh = 31, ox = -1, oy = -1, oz = -1;       // the cached octant: corner >> osh (none: no voxel of the volume has v >> 31 == -1)
      uint32_t ocls = SE_COLLIDE_EMPTY, oslot = 0u;
      for (int left = 3 * size + 8; left > 0; --left) {
        bool land = false;                           // cn / cd has jumped: v and the crossings are formed anew
        if (!in_volume(m, vx, vy, vz)) {
          st = min(st, SE_COLLIDE_UNSEEN);
          if (stop_at >= SE_COLLIDE_UNSEEN) { tn = cn; td = cd; fx = vx; fy = vy; fz = vz; break; }
          if (entered) break;
          int Ln = 0, Ld = 1, Un = 1, Ud = 1;
          bool hit = se_motion_axis(ax, ax, dx, 0, S, Ln, Ld, Un, Ud);
          hit = se_motion_axis(ay, ay, dy, 0, S, Ln, Ld, Un, Ud) && hit;
          hit = se_motion_axis(az, az, dz, 0, S, Ln, Ld, Un, Ud) && hit;
          if (!(hit && se_rat_less(Ln, Ld, Un, Ud))) break;     // the segment never enters the volume
          cn = Ln; cd = Ld; land = true;
          entered = true;                            // (whatever the landing gives, no second jump)
        } else {
          entered = true;
          if ((vx >> osh) != ox || (vy >> osh) != oy || (vz >> osh) != oz) {
            const int qx = vx >> 3, qy = vy >> 3, qz = vz >> 3;
            const uint32_t e = m.tab[leaf_index(m, qx, qy, qz)];
            if (e != 0u && e != SE_PENDING) {
              osh = 3; ocls = SE_TRACE_PRESENT;
              oslot = DENSE ? block_linear(m, qx, qy, qz) : e - 1u;
            } else {
              int sh;
              const size_t vs = absent_value_slot(m, qx, qy, qz, sh);
              ocls = se_collide_class(m.nx[vs], m.ny[vs], fc, thr, above);
              osh = 3 + sh;
            }
            ox = vx >> osh; oy = vy >> osh; oz = vz >> osh;
          }
          uint32_t cls = ocls;
          if (ocls == SE_TRACE_PRESENT) {
            const size_t vi = (size_t)oslot * SE_BRICK_STRIDE + (size_t)((vx & 7) + ((vy & 7) << 3) + ((vz & 7) << 6));
            cls = se_collide_class(m.vx[vi], se_ld_y(m, vi), fc, thr, above);
          }
          st = min(st, cls);
          if (cls <= stop_at) { tn = cn; td = cd; fx = vx; fy = vy; fz = vz; break; }
          if (COUNT) { cu += cls == SE_COLLIDE_UNSEEN ? 1 : 0; ce += cls == SE_COLLIDE_EMPTY ? 1 : 0; }
          if (!COUNT && ocls != SE_TRACE_PRESENT) {
            // nothing to count: the absent octant is left at its exit parameter
            int Ln = 0, Ld = 1, Un = 1, Ud = 1;
            const int s = 16 << osh;
            se_motion_axis(ax, ax, dx, ox << (osh + SE_TRACE_SUB_SHIFT), s, Ln, Ld, Un, Ud);
            se_motion_axis(ay, ay, dy, oy << (osh + SE_TRACE_SUB_SHIFT), s, Ln, Ld, Un, Ud);
            se_motion_axis(az, az, dz, oz << (osh + SE_TRACE_SUB_SHIFT), s, Ln, Ld, Un, Ud);
            if (!se_rat_less(Un, Ud, 1, 1)) break;              // the segment ends inside it
            cn = Un; cd = Ud; land = true;
          }
        }
        if (land) {
          vx = se_trace_land(ax, dx, cn, cd); vy = se_trace_land(ay, dy, cn, cd); vz = se_trace_land(az, dz, cn, cd);
          nx = se_trace_next(ax, dx, vx); ny = se_trace_next(ay, dy, vy); nz = se_trace_next(az, dz, vz);
          continue;
        }
        // a step: the smallest crossing parameter, every axis tied at it
        int mn = nx, md = adx;
        if (se_rat_less(ny, ady, mn, md)) { mn = ny; md = ady; }
        if (se_rat_less(nz, adz, mn, md)) { mn = nz; md = adz; }
        if (mn >= md) break;                         // not below 1: the segment ends in this voxel
        const bool mx = !se_rat_less(mn, md, nx, adx), my = !se_rat_less(mn, md, ny, ady), mz = !se_rat_less(mn, md, nz, adz);
        cn = mn; cd = md;
        if (mx) { vx += sx; nx += 16; }
        if (my) { vy += sy; ny += 16; }
        if (mz) { vz += sz; nz += 16; }
      }
    }
    a.status[i] = (uint8_t)st;
    if (a.t_first) a.t_first[i] = (float)tn / (float)td;
    if (a.first) { a.first[3 * i] = fx; a.first[3 * i + 1] = fy; a.first[3 * i + 2] = fz; }
    if (COUNT) { a.counts[2 * i] = cu; a.counts[2 * i + 1] = ce; }
  }
}
