// Column projections of the resident map (se_hip_project_columns, include/se_hip.h): for a footprint [lo, lo + side) on two axes (u the lower
// axis and the fastest output index, v the other) and L half-open intervals [a_l, b_l) along the third axis w, per cell (l, j, i) -- the
// voxels with u = lo_u + i, v = lo_v + j, w in [a_l, b_l) -- the min class over the cell's voxels (status), the smallest and the largest w of
// a blocking voxel (first, last) and the number of blocking voxels (count).  A voxel is classified as k_collide_boxes classifies it in strict
// mode: classify(Octree::get(v)) inside [0, size)^3 (a pending index entry counts as absent), unseen outside; it blocks when its class is
// <= stop_at.  The host restatement and the literal definition are include/se/project_columns.hpp.
//
// One wave64 per (block-aligned 8 x 8 tile of the footprint, layer), grid-stride over the tiles; the lanes are the tile's 64 columns, lane =
// (u & 7) + 8 (v & 7); a lane outside a ragged footprint edge computes with the others and writes nothing.  Control flow is wave-uniform: the
// tile's block column and the position w are the same in every lane.
//   - the wave walks [a, b) ∩ [0, size) upwards in octant steps.  At w it reads the leaf entry of tab[]; a present block gives every lane the
//     up to 8 voxels of its column (loads issued together, then classified), and the walk goes on at the block's end;
//   - an absent block: the index pyramid is read top-down to the first absent octant on the path, as Octree::get does.  Its side s and its
//     parent's value_[child] answer [w0, w0 + s) ∩ [a, b) for all 64 columns at once -- exact, because every voxel of an absent octant reads
//     that one value, and the 8 x 8 tile lies inside the octant (s >= 8, both aligned) -- and the walk goes on at w0 + s;
//   - the parts of [a, b) below 0 and from size on, and the whole of [a, b) for a tile outside the volume in u or v (the volume's side is a
//     multiple of 8, so a tile is inside or outside as a whole), are unseen and answered in closed form: no loop over them.
// Every loop is bounded by the structure: a step of the walk advances w by at least 8 - (w & 7) >= 1 to a multiple of 8, so a wave makes at
// most size / 8 steps, each with at most leaf_level index reads; the grid-stride loop ends with the tile count.  Each lane writes its own
// cell: no atomics.  Brick reads stay inside the brick of a present block, index reads inside the pyramid (block coordinates are checked
// against the volume before the walk), node reads at value_[0..7] of an existing node.
// Brick layout per axis (voxel x + 8 y + 64 z): along z a column's voxels are 64 floats apart and its SDF weight bytes are one 8-byte word
// (SE_YB); along y they are 8 floats apart; along x they are 8 consecutive floats, loaded as a whole whatever part of them is asked for.
#pragma once
#include "se_collide_kernels.h"

#define SE_PROJECT_LIMIT (1 << 20)       // lo, lo + side, a and b within [-2^20, 2^20], else the request is invalid
#define SE_PROJECT_MAX_LAYERS 16
#define SE_PROJECT_NONE ((int32_t)0x80000000)

struct ProjectArgs {
  int lo_u, lo_v, side_u, side_v;
  int n_layers;
  int layers[SE_PROJECT_MAX_LAYERS][2];
  uint8_t* status; int32_t* first; int32_t* last; int32_t* count;
  float thr; int above; uint32_t stop_at;
};

// A lane's running answer over the part of its column walked so far (the walk ascends: `last` is simply overwritten).
struct SeProjectCell { uint32_t st; int first, last, count; };

// the stretch [r0, r1) of one class for every column of the tile
__device__ __forceinline__ void se_project_run(SeProjectCell& c, uint32_t cls, uint32_t stop_at, int r0, int r1) {
  if (r0 >= r1) return;
  c.st = min(c.st, cls);
  if (cls <= stop_at) {
    c.first = min(c.first, r0);
    c.last = r1 - 1;
    c.count += r1 - r0;
  }
}

// The voxels [k0, k1) of the lane's column in the present block at `slot`, whose first voxel along the axis has coordinate w0.
template <int AXIS>
__device__ __forceinline__ void se_project_block(const DevMap& m, const FieldConst fc, float thr, int above, uint32_t stop_at, uint32_t slot, int w0, int k0, int k1,
                                                 SeProjectCell& c) {
  const uint32_t lane = threadIdx.x & 63u;
  // the column's first voxel and the step along the axis
  const uint32_t vb = AXIS == 2 ? lane : (AXIS == 1 ? (lane & 7u) + ((lane >> 3) << 6) : lane << 3);
  const uint32_t vs = AXIS == 2 ? 64u : (AXIS == 1 ? 8u : 1u);
  const float* brick = m.vx + (size_t)slot * SE_BRICK_STRIDE;
  float vx[8], vy[8];
  if (m.ybyte) {
    const uint8_t* wt = (const uint8_t*)(brick + 512);
    if (AXIS == 2) {   // SE_YB(lane + 64 k) = 8 lane + k: the column's weights are one aligned 8-byte word
      const uint2 wv = *(const uint2*)(wt + (lane << 3));
#pragma unroll
      for (int k = 0; k < 8; ++k) vy[k] = (float)(((k < 4 ? wv.x : wv.y) >> (8 * (k & 3))) & 0xFFu);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        vx[k] = fc.init_x;
        if (k >= k0 && k < k1) vx[k] = brick[vb + (uint32_t)k * vs];
      }
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        vx[k] = fc.init_x; vy[k] = fc.init_y;
        if (AXIS == 0 || (k >= k0 && k < k1)) {
          const uint32_t v = vb + (uint32_t)k * vs;
          vx[k] = brick[v]; vy[k] = (float)wt[SE_YB(v)];
        }
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      vx[k] = fc.init_x; vy[k] = fc.init_y;
      if (AXIS == 0 || (k >= k0 && k < k1)) {
        const uint32_t v = vb + (uint32_t)k * vs;
        vx[k] = brick[v]; vy[k] = brick[512u + v];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    if (k >= k0 && k < k1) {
      const uint32_t cls = se_collide_class(vx[k], vy[k], fc, thr, above);
      c.st = min(c.st, cls);
      if (cls <= stop_at) {
        c.first = min(c.first, w0 + k);
        c.last = w0 + k;
        c.count += 1;
      }
    }
  }
}

template <bool DENSE, int AXIS>
__global__ __launch_bounds__(SE_WG_COLLIDE) void k_project_columns(DevMap m, ProjectArgs a) {
  const FieldConst fc = se_field_const(m);
  const int lane = (int)(threadIdx.x & 63u);
  const float thr = a.thr;
  const int above = a.above;
  const uint32_t stop_at = a.stop_at;
  const int leaf = m.leaf_level, size = m.size, nb = m.size >> 3;
  // the tiles: block-aligned, from the one that holds lo to the one that holds lo + side - 1 (>> 3 floors for negative coordinates too)
  const int tu0 = a.lo_u >> 3, tv0 = a.lo_v >> 3;
  const long long ntu = ((a.lo_u + a.side_u - 1) >> 3) - tu0 + 1, ntv = ((a.lo_v + a.side_v - 1) >> 3) - tv0 + 1;
  const long long n_items = ntu * ntv * a.n_layers;

  for (long long it = blockIdx.x; it < n_items; it += gridDim.x) {
    const int layer = (int)(it / (ntu * ntv));
    const long long tile = it - (long long)layer * (ntu * ntv);
    const int bu = tu0 + (int)(tile % ntu), bv = tv0 + (int)(tile / ntu);   // the tile's block column
    const int wa = a.layers[layer][0], wb = a.layers[layer][1];
    const int u = bu * 8 + (lane & 7), v = bv * 8 + (lane >> 3);
    const bool active = u >= a.lo_u && u < a.lo_u + a.side_u && v >= a.lo_v && v < a.lo_v + a.side_v;
    SeProjectCell c = {SE_COLLIDE_EMPTY, 0x7FFFFFFF, SE_PROJECT_NONE, 0};
    const bool inside = (unsigned)bu < (unsigned)nb && (unsigned)bv < (unsigned)nb;
    if (!inside) {
      se_project_run(c, SE_COLLIDE_UNSEEN, stop_at, wa, wb);
    } else {
      se_project_run(c, SE_COLLIDE_UNSEEN, stop_at, wa, min(wb, 0));
      const int wend = min(wb, size);
      int w = max(wa, 0);
      while (w < wend) {
        const int bw = w >> 3;
        const int bx = AXIS == 0 ? bw : bu, by = AXIS == 0 ? bu : (AXIS == 1 ? bw : bv), bz = AXIS == 2 ? bw : bv;
        const uint32_t e = m.tab[leaf_index(m, bx, by, bz)];
        if (e != 0u && e != SE_PENDING) {
          const uint32_t slot = DENSE ? block_linear(m, bx, by, bz) : e - 1u;
          se_project_block<AXIS>(m, fc, thr, above, stop_at, slot, bw * 8, w - bw * 8, min(wend, bw * 8 + 8) - bw * 8, c);
          w = bw * 8 + 8;
        } else {
          // Octree::get: the walk of absent_value_slot (se_device.h), kept as its own copy here: calling the helper cost this kernel 2 - 3 %
          uint32_t nid = 0u;
          int lmiss = leaf;
          bool down = true;
#pragma unroll
          for (int l = 1; l < SE_MAX_LEVELS; ++l) {
            if (down && l < leaf) {
              const int sh = leaf - l;
              const uint32_t t = m.tab[tab_index(m, l, bx >> sh, by >> sh, bz >> sh)];
              if (t != 0u && t != SE_PENDING) nid = t - 1u;
              else { lmiss = l; down = false; }
            }
          }
          const int sh = leaf - lmiss;
          const uint32_t child = ((uint32_t)(bx >> sh) & 1u) | (((uint32_t)(by >> sh) & 1u) << 1) | (((uint32_t)(bz >> sh) & 1u) << 2);
          const uint32_t cls = se_collide_class(m.nx[(size_t)nid * 8 + child], m.ny[(size_t)nid * 8 + child], fc, thr, above);
          const int s = 8 << sh;                 // the absent octant's side, and its end along the axis
          const int w1 = (w & ~(s - 1)) + s;
          se_project_run(c, cls, stop_at, w, min(w1, wend));
          w = w1;
        }
      }
      se_project_run(c, SE_COLLIDE_UNSEEN, stop_at, max(wa, size), wb);
    }
    if (active) {
      const size_t o = ((size_t)layer * (size_t)a.side_v + (size_t)(v - a.lo_v)) * (size_t)a.side_u + (size_t)(u - a.lo_u);
      a.status[o] = (uint8_t)c.st;
      if (a.first) a.first[o] = c.count ? c.first : SE_PROJECT_NONE;
      if (a.last) a.last[o] = c.count ? c.last : SE_PROJECT_NONE;
      if (a.count) a.count[o] = c.count;
    }
  }
}
