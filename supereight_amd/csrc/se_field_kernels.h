// The distance field of a map region (se_hip_distance_field, include/se_hip.h): for every voxel v of the region [lo, lo + side) the answer of
// se_hip_clearance_boxes to the query (v, robot, r_max) -- the squared distance d2 from the box [v, v + robot) to the nearest blocking voxel
// within r_max, and that voxel, among the nearest ones the smallest in (z, y, x) order -- bit for bit.  Classification, gap formula and tie
// rule are those of se_clearance_kernels.h; the host restatement and the literal definition are include/se/distance_field.hpp.
//
// The gap is per axis, g_k(c) = max(0, c_k - (v_k + robot_k), v_k - (c_k + 1)), so d2 = g_x^2 + g_y^2 + g_z^2 is a min-plus product and the
// field separates into three 1-D passes.  With o = c - v the gap is g(o) = max(0, o - robot, -o - 1): zero on o in [-1, robot], and at most
// r_max exactly on o in [-1 - r_max, robot + r_max].  A candidate with d2 <= r_max^2 has every gap <= r_max, so per axis only the domain
//     [lo_k - 1 - r_max, lo_k + side_k - 1 + robot_k + r_max],   D_k = side_k + robot_k + 2 r_max + 1 cells,
// is ever looked at.  Four plain launches on the handle's stream, no atomics, nothing shared between workgroups:
//   k_field_classify  one wave64 per 8^3 cell of the block-aligned hull of the domain (grid-stride over the cells), on the walk of
//                     k_project_columns with AXIS == 0: lane = (y, z) of the cell, the lane's 8 x-voxels loaded together and classified with
//                     se_collide_class.  A present block gives one byte of blocking bits per lane; an absent octant (value_[child] of the
//                     deepest existing node) and a cell outside [0, size)^3 (unseen) are answered as a whole cell, 0x00 or 0xFF.  The bytes
//                     go into bit rows along x: row (z, y) of the hull is `words` 64-bit words, bit p of the row is the voxel x = 8 bx0 + p
//                     (little-endian: byte b of a word holds bits 8 b .. 8 b + 7).  Rows instead of the 64 contiguous bytes per block that a
//                     block-major layout would give: k_field_x then reads whole words of one row and needs no gather across blocks.  The
//                     two layouts were not measured against each other; classify is 4 to 12 % of a 128^3 call.
//   k_field_x         one lane per (i, y', z') of side_x * D_y * D_z: the lowest set bit of the row inside the zero-gap interval
//                     [v - 1, v + robot]; else the nearest set bit below (within r_max) and above (within r_max), the lower one at equal
//                     gaps.  64-bit ctz / clz over masked words; each of the three searches reads at most ceil(span / 64) + 1 words, span
//                     <= robot + 2 <= 258 resp. r_max <= 255.  Writes the offset c_x - v_x as int16, or SE_FIELD_NO16.
//   k_field_y         one lane per (i, j, z') of side_x * side_y * D_z, lanes along x (every read and write coalesced): scans its window of
//                     robot_y + 2 r_max + 2 candidates c_y ascending, straight from L2 (neighbouring lanes read neighbouring entries and
//                     neighbouring j share all but one row, so an LDS copy would save no DRAM traffic; not measured against one: this pass is 35 to 63 % of a
//                     128^3 call), keeps
//                     the first strict minimum of g_x^2 + g_y^2 -- the lowest c_y at equal cost, with the c_x that k_field_x chose for that
//                     row: the lexicographic minimum of (cost, c_y, c_x).  Writes both offsets packed in 32 bits, or SE_FIELD_NO32.
//   k_field_z         one lane per voxel (i, j, k): the same scan over robot_z + 2 r_max + 2 candidates c_z; the first strict minimum is the
//                     lexicographic minimum of (d2, c_z, c_y, c_x), because a candidate that is not minimal in its own line cannot attain
//                     the minimum of the sum.  Applies d2 <= r_max^2, writes d2 and, where asked for, nearest = v + offsets.
// Every loop is bounded by the request: the grid-stride loops by the cell count resp. the lane count (<= 2^28, checked by the host), the absent
// octant's descent by leaf_level, the word loops by the three spans above, the window loops by robot + 2 r_max + 2 <= 768.  Every index is
// formed in size_t from quantities the host has checked.  Brick reads happen only for a present entry (e != 0 && e != SE_PENDING), index
// reads only for block coordinates inside the volume.  The searches of k_field_x stay inside the row: their bit range lies inside the domain,
// the domain inside the hull.  No LDS.
#pragma once
#include "se_collide_kernels.h"

#define SE_FIELD_LIMIT (1 << 19)        // lo and lo + side + robot within [-2^19, 2^19]: every voxel's query is a valid clearance query
#define SE_FIELD_RMAX 255               // r_max within [0, 255]
#define SE_FIELD_ROBOT 256              // robot side within [1, 256]
#define SE_FIELD_MAX_VOXELS (1ll << 24) // side_x * side_y * side_z
#define SE_FIELD_MAX_WORK (1ll << 28)   // side_x * D_y * D_z: the entries of the x pass's buffer
#define SE_FIELD_NONE (-1)
#define SE_FIELD_NO16 ((int16_t)-32768)
#define SE_FIELD_NO32 0x80008000u
#define SE_WG_FIELD 256

// What k_field_classify reads and writes: the block-aligned hull of a domain and the occupancy test.
struct HullArgs {
  int b0[3], nb[3];              // the hull in blocks: first block and block count per axis
  int words;                     // 64-bit words per bit row: ceil(nb[0] / 8)
  unsigned long long* bits;      // [8 nb[2]][8 nb[1]][words]
  float thr; int above; uint32_t stop_at;
};
struct FieldArgs {
  int lo[3], side[3], robot[3];
  int r_max;
  int D[3];                      // the domain's cells per axis
  HullArgs hull;
  int16_t* ax;                   // [D[2]][D[1]][side[0]]
  uint32_t* ay;                  // [D[2]][side[1]][side[0]]
  int32_t* d2; int32_t* nearest; // [side[2]][side[1]][side[0]] (nearest: [3] more)
};

// the gap of a candidate at offset o = c - v from a box of side `robot` at v
__device__ __forceinline__ int se_field_gap(int o, int robot) { return max(max(o - robot, -o - 1), 0); }

template <bool DENSE>
__global__ __launch_bounds__(SE_WG_COLLIDE) void k_field_classify(DevMap m, HullArgs a) {
  const FieldConst fc = se_field_const(m);
  const uint32_t lane = threadIdx.x & 63u;
  const float thr = a.thr;
  const int above = a.above;
  const uint32_t stop_at = a.stop_at;
  const int nb = m.size >> 3;
  const size_t n0 = (size_t)a.nb[0], n1 = (size_t)a.nb[1], cells = n0 * n1 * (size_t)a.nb[2];
  const size_t row_bytes = (size_t)a.words * 8u;
  uint8_t* out = (uint8_t*)a.bits;
  for (size_t it = blockIdx.x; it < cells; it += gridDim.x) {
    const size_t ix = it % n0, iy = (it / n0) % n1, iz = it / (n0 * n1);
    const int bx = a.b0[0] + (int)ix, by = a.b0[1] + (int)iy, bz = a.b0[2] + (int)iz;
    uint32_t byte;
    if (!((unsigned)bx < (unsigned)nb && (unsigned)by < (unsigned)nb && (unsigned)bz < (unsigned)nb)) {
      byte = SE_COLLIDE_UNSEEN <= stop_at ? 0xFFu : 0u;   // (the volume's side is a multiple of 8: a cell is inside or outside as a whole)
    } else {
      const uint32_t e = m.tab[leaf_index(m, bx, by, bz)];
      if (e != 0u && e != SE_PENDING) {
        const uint32_t slot = DENSE ? block_linear(m, bx, by, bz) : e - 1u;
        const float* brick = m.vx + (size_t)slot * SE_BRICK_STRIDE;
        const uint32_t vb = lane << 3;   // the lane's row: voxel x + 8 y + 64 z, y = lane & 7, z = lane >> 3
        float vx[8], vy[8];
        if (m.ybyte) {
          const uint8_t* wt = (const uint8_t*)(brick + 512);
#pragma unroll
          for (int k = 0; k < 8; ++k) { vx[k] = brick[vb + (uint32_t)k]; vy[k] = (float)wt[SE_YB(vb + (uint32_t)k)]; }
        } else {
#pragma unroll
          for (int k = 0; k < 8; ++k) { vx[k] = brick[vb + (uint32_t)k]; vy[k] = brick[512u + vb + (uint32_t)k]; }
        }
        byte = 0u;
#pragma unroll
        for (int k = 0; k < 8; ++k) byte |= (se_collide_class(vx[k], vy[k], fc, thr, above) <= stop_at ? 1u : 0u) << k;
      } else {
        int sh;   // Octree::get: the value of the first missing octant on the block's path (absent_value_slot, se_device.h)
        const size_t vs = absent_value_slot(m, bx, by, bz, sh);
        const uint32_t cls = se_collide_class(m.nx[vs], m.ny[vs], fc, thr, above);
        byte = cls <= stop_at ? 0xFFu : 0u;
      }
    }
    const size_t row = (iz * 8u + (size_t)(lane >> 3)) * (n1 * 8u) + (iy * 8u + (size_t)(lane & 7u));
    out[row * row_bytes + ix] = (uint8_t)byte;
  }
}

// the lowest set bit of the row within [from, to] (bit positions, from <= to inside the row), or -1; at most (to - from) / 64 + 2 words
__device__ __forceinline__ int se_field_lowest(const unsigned long long* row, int from, int to) {
  for (int w = from >> 6; w <= (to >> 6); ++w) {
    unsigned long long v = row[w];
    if (w == (from >> 6)) v &= ~0ull << (from & 63);
    if (w == (to >> 6)) v &= ~0ull >> (63 - (to & 63));
    if (v) return w * 64 + (int)__builtin_ctzll(v);
  }
  return -1;
}
// the highest one
__device__ __forceinline__ int se_field_highest(const unsigned long long* row, int from, int to) {
  for (int w = to >> 6; w >= (from >> 6); --w) {
    unsigned long long v = row[w];
    if (w == (from >> 6)) v &= ~0ull << (from & 63);
    if (w == (to >> 6)) v &= ~0ull >> (63 - (to & 63));
    if (v) return w * 64 + 63 - (int)__builtin_clzll(v);
  }
  return -1;
}

__global__ __launch_bounds__(SE_WG_FIELD) void k_field_x(FieldArgs a) {
  const size_t s0 = (size_t)a.side[0], d1 = (size_t)a.D[1], total = s0 * d1 * (size_t)a.D[2];
  const int r = a.r_max, robot = a.robot[0];
  // the domain's origin inside the hull, per axis: (lo - 1 - r_max) - 8 b0, in [0, 8)
  const int hx = a.lo[0] - 1 - r - 8 * a.hull.b0[0], hy = a.lo[1] - 1 - r - 8 * a.hull.b0[1], hz = a.lo[2] - 1 - r - 8 * a.hull.b0[2];
  const size_t rows_y = (size_t)a.hull.nb[1] * 8u;
  for (size_t idx = (size_t)blockIdx.x * SE_WG_FIELD + threadIdx.x; idx < total; idx += (size_t)gridDim.x * SE_WG_FIELD) {
    const size_t i = idx % s0, y = (idx / s0) % d1, z = idx / (s0 * d1);
    const unsigned long long* row = a.hull.bits + ((z + (size_t)hz) * rows_y + (y + (size_t)hy)) * (size_t)a.hull.words;
    const int pv = hx + 1 + r + (int)i;   // the bit of v_x = lo_x + i
    int c = se_field_lowest(row, pv - 1, pv + robot);
    if (c < 0 && r > 0) {
      const int below = se_field_highest(row, pv - 1 - r, pv - 2), up = se_field_lowest(row, pv + robot + 1, pv + robot + r);
      // gaps: pv - 1 - below and up - (pv + robot); the lower voxel at equal gaps
      if (below >= 0 && (up < 0 || pv - 1 - below <= up - pv - robot)) c = below;
      else c = up;
    }
    a.ax[idx] = c < 0 ? SE_FIELD_NO16 : (int16_t)(c - pv);
  }
}

__global__ __launch_bounds__(SE_WG_FIELD) void k_field_y(FieldArgs a) {
  const size_t s0 = (size_t)a.side[0], s1 = (size_t)a.side[1], d1 = (size_t)a.D[1], total = s0 * s1 * (size_t)a.D[2];
  const int r = a.r_max, rx = a.robot[0], ry = a.robot[1], window = ry + 2 * r + 2;
  for (size_t idx = (size_t)blockIdx.x * SE_WG_FIELD + threadIdx.x; idx < total; idx += (size_t)gridDim.x * SE_WG_FIELD) {
    const size_t i = idx % s0, j = (idx / s0) % s1, z = idx / (s0 * s1);
    const int16_t* col = a.ax + (z * d1 + j) * s0 + i;   // the candidate c_y = v_y - 1 - r_max + t is row j + t of the domain
    int best = 0x7FFFFFFF;
    uint32_t pair = SE_FIELD_NO32;
    for (int t = 0; t < window; ++t) {
      const int ox = col[(size_t)t * s0];
      if (ox == SE_FIELD_NO16) continue;
      const int oy = t - 1 - r, gx = se_field_gap(ox, rx), gy = se_field_gap(oy, ry);
      const int cost = gx * gx + gy * gy;
      if (cost < best) { best = cost; pair = ((uint32_t)(uint16_t)(int16_t)oy << 16) | (uint32_t)(uint16_t)(int16_t)ox; }
    }
    a.ay[idx] = pair;
  }
}

__global__ __launch_bounds__(SE_WG_FIELD) void k_field_z(FieldArgs a) {
  const size_t s0 = (size_t)a.side[0], s1 = (size_t)a.side[1], plane = s0 * s1, total = plane * (size_t)a.side[2];
  const int r = a.r_max, rx = a.robot[0], ry = a.robot[1], rz = a.robot[2], window = rz + 2 * r + 2;
  for (size_t idx = (size_t)blockIdx.x * SE_WG_FIELD + threadIdx.x; idx < total; idx += (size_t)gridDim.x * SE_WG_FIELD) {
    const size_t i = idx % s0, j = (idx / s0) % s1, k = idx / plane;
    const uint32_t* col = a.ay + k * plane + j * s0 + i;   // the candidate c_z = v_z - 1 - r_max + t is plane k + t of the domain
    int best = 0x7FFFFFFF, bx = 0, by = 0, bz = 0;
    for (int t = 0; t < window; ++t) {
      const uint32_t pr = col[(size_t)t * plane];
      if (pr == SE_FIELD_NO32) continue;
      const int ox = (int)(int16_t)(uint16_t)(pr & 0xFFFFu), oy = (int)(int16_t)(uint16_t)(pr >> 16), oz = t - 1 - r;
      const int gx = se_field_gap(ox, rx), gy = se_field_gap(oy, ry), gz = se_field_gap(oz, rz);
      const int cost = gx * gx + gy * gy + gz * gz;
      if (cost < best) { best = cost; bx = ox; by = oy; bz = oz; }
    }
    const bool found = best <= r * r;
    a.d2[idx] = found ? best : SE_FIELD_NONE;
    if (a.nearest) {
      a.nearest[3 * idx + 0] = found ? a.lo[0] + (int)i + bx : (int32_t)0x80000000;
      a.nearest[3 * idx + 1] = found ? a.lo[1] + (int)j + by : (int32_t)0x80000000;
      a.nearest[3 * idx + 2] = found ? a.lo[2] + (int)k + bz : (int32_t)0x80000000;
    }
  }
}
