// Merge of one resident map into another (se_hip_merge_map, include/se_hip.h): source content at voxel c meets destination content at c + s and is
// combined value by value (se_merge_value below; the host restatement is se::merge_value / se::merge_map of include/se/merge_map.hpp).  One kernel
// holds both maps: DevMap travels by value.  The source is only read; the two maps are distinct allocations.
//   k_merge_select   a lane per source block-list entry and per source node entry: does it take part, its key in the destination; the participants of
//                    a wave are compacted with se_wave_take into two key lists in the destination's staging, each with its source list position;
//                    the destination voxel box of the participating blocks is reduced per wave (at most six atomics per wave), and the nodes that
//                    the destination does not hold yet are counted (one atomic per wave)
//   (host)           k_alloc_commit on the destination over the node list, then the block list: tab[], occ[], lbits[], cbits[], fbits[], the lists
//                    and the counters are those of a map that was allocated that way, missing ancestors included
//   k_merge_bricks   the hot path, a wave per participating block: lane l owns the column of voxels l + 64 z, as the sweep does -- eight coalesced
//                    float loads per brick, and for SDF the column's eight byte weights as ONE 8-byte access at 8 l (SE_YB is the same on both
//                    sides); every value of the destination brick is stored back, changed or not (the only form measured); lane 0 ORs bactive[].
//                    The slot of either brick is looked up, never assumed: the destination's from tab[] in both layouts (dense: tab[] holds the
//                    grid position + 1 -- one wave-uniform load per 8 KiB of traffic buys the proof that the block was inserted), the source's by
//                    block_slot from its list.  Node values by key, a lane per value_[j], in the same launch
#pragma once
#include "se_kernels.h"

#define SE_MERGE_FUSE 0
#define SE_MERGE_REPLACE 1
#define SE_MERGE_FILL 2
#define SE_MERGE_ROOT 0ull        // node-list entry of the source root (key 0: level 0): k_alloc_commit skips it, the root always exists

struct MergeArgs {
  int s[3];                      // voxels, multiples of 8
  int mode;                      // SE_MERGE_*
  float max_weight;              // SDF: an integer in [1, 255]
  int dlevel;                    // destination level of a source node = its source level + dlevel (the sizes may differ)
  uint32_t nb, nn;               // blocks / nodes (root included) of the source, never more than its pools hold
  unsigned long long* blist;     // [count, key ...]: destination keys of the participating blocks
  unsigned long long* nlist;     // ... of the participating nodes
  unsigned long long* ncreated;  // participating nodes that the destination did not hold
  uint32_t* bsrc;                // [nb] source list position, in the order of blist
  uint32_t* nsrc;                // [nn] ... of nlist
  int* box;                      // lo[3] (start: INT_MAX), hi[3] (start: INT_MIN): corners of the participating blocks in the destination, min and max + 8
};

// a = destination, b = source; the definition is the table of include/se_hip.h
template <bool OFUSION>
__device__ __forceinline__ void se_merge_value(float& ax, float& ay, float bx, float by, int mode, float maxw, float ix, float iy) {
  if (bx == ix && by == iy) return;
  const float ty = OFUSION ? by : fminf(by, maxw);
  if ((ax == ix && ay == iy) || mode == SE_MERGE_REPLACE) { ax = bx; ay = ty; return; }
  if (mode == SE_MERGE_FILL) return;
  if (OFUSION) {
    ax = clampf(ax + bx, -1000.f, 1000.f);
    ay = fmaxf(ay, by);
  } else {
    if (by == 0.f) return;
    if (ay == 0.f) { ax = bx; ay = ty; return; }
    const float w = ay + by;
    ax = clampf((ay * ax + by * bx) / w, -1.f, 1.f);
    ay = fminf(w, maxw);
  }
}

__device__ __forceinline__ int se_wave_min(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int se_wave_max(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// d = destination, m = source
__global__ __launch_bounds__(SE_WG) void k_merge_select(DevMap d, DevMap m, MergeArgs a) {
  const uint32_t n = max(a.nb, a.nn);
  const uint32_t rounds = (n + gridDim.x * SE_WG - 1) / (gridDim.x * SE_WG);   // every lane of a wave makes every round (ballots, shuffles)
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t r = 0; r < rounds; ++r) {
    const uint32_t i = (r * gridDim.x + blockIdx.x) * SE_WG + threadIdx.x;
    {
      // block i: its corner + s within [0, dst size - 8] on every axis
      const bool is_block = i < a.nb;
      const uint32_t bp = is_block ? m.bpos[i] : 0u;
      const int nblk = 1 << d.leaf_level;
      const int x = (int)(bp & 1023u) + (a.s[0] >> 3), y = (int)((bp >> 10) & 1023u) + (a.s[1] >> 3), z = (int)(bp >> 20) + (a.s[2] >> 3);
      const bool keep = is_block && (unsigned)x < (unsigned)nblk && (unsigned)y < (unsigned)nblk && (unsigned)z < (unsigned)nblk;
      const unsigned long long at = se_wave_take(&a.blist[0], keep);
      if (keep) {
        a.blist[1 + at] = se_make_key(x, y, z, d.leaf_level, d.max_level);
        a.bsrc[at] = i;
      }
      if (__ballot(keep) != 0ull) {
        const int big = 0x7FFFFFFF;
        const int lx = se_wave_min(keep ? x : big), ly = se_wave_min(keep ? y : big), lz = se_wave_min(keep ? z : big);
        const int hx = se_wave_max(keep ? x : -1), hy = se_wave_max(keep ? y : -1), hz = se_wave_max(keep ? z : -1);
        if (lane == 0u) {
          atomicMin(&a.box[0], lx * 8); atomicMin(&a.box[1], ly * 8); atomicMin(&a.box[2], lz * 8);
          atomicMax(&a.box[3], hx * 8 + 8); atomicMax(&a.box[4], hy * 8 + 8); atomicMax(&a.box[5], hz * 8 + 8);
        }
      }
    }
    {
      // node i of side dd: s a multiple of dd on every axis and its corner + s within [0, dst size - dd]; the source root (i = 0) only for s = 0 and equal sizes
      const bool is_node = i < a.nn;
      const int slevel = is_node ? (int)m.nlevel[i] : 0;
      const uint32_t np = is_node ? m.npos[i] : 0u;
      const int level = slevel + a.dlevel;                   // in the destination
      const int sh = m.max_level - slevel;                   // log2 of the side (voxels), the same in both maps
      const int low = (1 << sh) - 1;
      const bool aligned = ((a.s[0] | a.s[1] | a.s[2]) & low) == 0;
      const int x = (int)(np & 1023u) + (a.s[0] >> sh), y = (int)((np >> 10) & 1023u) + (a.s[1] >> sh), z = (int)(np >> 20) + (a.s[2] >> sh);
      const bool lvl_ok = slevel >= 1 ? (level >= 0 && level < d.leaf_level && slevel < m.leaf_level) : (a.dlevel == 0 && (a.s[0] | a.s[1] | a.s[2]) == 0);
      const int cells = 1 << (level < 0 ? 0 : level);
      const bool keep = is_node && lvl_ok && aligned && (unsigned)x < (unsigned)cells && (unsigned)y < (unsigned)cells && (unsigned)z < (unsigned)cells;
      const unsigned long long at = se_wave_take(&a.nlist[0], keep);
      bool fresh = false;
      if (keep) {
        a.nlist[1 + at] = level == 0 ? SE_MERGE_ROOT : se_make_key(x, y, z, level, d.max_level);
        a.nsrc[at] = i;
        fresh = level != 0 && d.tab[tab_index(d, level, x, y, z)] == 0u;
      }
      const unsigned long long fm = __ballot(fresh);
      if (fm != 0ull && lane == (uint32_t)__builtin_ctzll(fm)) atomicAdd(a.ncreated, (unsigned long long)__builtin_popcountll(fm));
    }
  }
}

template <bool OFUSION>
__global__ __launch_bounds__(SE_WG) void k_merge_bricks(DevMap d, DevMap m, MergeArgs a) {
  const uint32_t lane = threadIdx.x & 63u, nwaves = gridDim.x * (SE_WG / 64);
  const uint32_t kept = (uint32_t)min(a.blist[0], (unsigned long long)a.nb);
  const int bsh = d.max_level - d.leaf_level;
  const int mode = a.mode;
  const float maxw = a.max_weight, ix = d.init_x, iy = d.init_y;
  for (uint32_t i = blockIdx.x * (SE_WG / 64) + (threadIdx.x >> 6); i < kept; i += nwaves) {
    const unsigned long long code = a.blist[1 + i] & ~0x1FFull;
    const int x = (int)(se_compact21(code) >> bsh), y = (int)(se_compact21(code >> 1) >> bsh), z = (int)(se_compact21(code >> 2) >> bsh);
    const uint32_t e = d.tab[leaf_index(d, x, y, z)];
    if (e == 0u || e == SE_PENDING) continue;   // (the pool ran out while the list was inserted: reported by the call)
    const uint32_t si = min(a.bsrc[i], a.nb - 1u);
    const uint32_t sslot = block_slot(m, si, m.bpos[si]);
    float* __restrict__ pa = d.vx + (size_t)(e - 1u) * SE_BRICK_STRIDE;
    const float* __restrict__ pb = m.vx + (size_t)sslot * SE_BRICK_STRIDE;
    float ax[8], ay[8], bx[8], by[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { ax[k] = pa[lane + 64 * k]; bx[k] = pb[lane + 64 * k]; }
    if (OFUSION) {
#pragma unroll
      for (int k = 0; k < 8; ++k) { ay[k] = pa[512 + lane + 64 * k]; by[k] = pb[512 + lane + 64 * k]; }
    } else {
      const uint2 wa = ((const uint2*)(pa + 512))[lane], wb = ((const uint2*)(pb + 512))[lane];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        ay[k] = (float)(((k < 4 ? wa.x : wa.y) >> (8 * (k & 3))) & 0xFFu);
        by[k] = (float)(((k < 4 ? wb.x : wb.y) >> (8 * (k & 3))) & 0xFFu);
      }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) se_merge_value<OFUSION>(ax[k], ay[k], bx[k], by[k], mode, maxw, ix, iy);
#pragma unroll
    for (int k = 0; k < 8; ++k) pa[lane + 64 * k] = ax[k];
    if (OFUSION) {
#pragma unroll
      for (int k = 0; k < 8; ++k) pa[512 + lane + 64 * k] = ay[k];
    } else {
      uint2 w = {0u, 0u};
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const uint32_t byte = (uint32_t)(int)ay[k] << (8 * (k & 3));   // (an integer in 0 .. 255: sums of byte weights, capped at max_weight <= 255)
        if (k < 4) w.x |= byte; else w.y |= byte;
      }
      ((uint2*)(pa + 512))[lane] = w;
    }
    if (lane == 0u && m.bactive[sslot]) d.bactive[e - 1u] = 1;
  }
  // the nodes: a lane per value_[j], by key as k_load_nodes writes them (node values are floats in both field types)
  const unsigned long long nkept = min(a.nlist[0], (unsigned long long)a.nn);
  for (unsigned long long i = blockIdx.x * (unsigned long long)SE_WG + threadIdx.x; i < nkept * 8; i += (unsigned long long)gridDim.x * SE_WG) {
    const unsigned long long key = a.nlist[1 + (i >> 3)];
    const int level = (int)(key & 0x1FFull);
    uint32_t nid = 0u;   // key 0 = the root
    if (level != 0) {
      if (level >= d.leaf_level) continue;
      const unsigned long long code = key & ~0x1FFull;
      const int sh = d.max_level - level;
      const int x = (int)(se_compact21(code) >> sh), y = (int)(se_compact21(code >> 1) >> sh), z = (int)(se_compact21(code >> 2) >> sh);
      if ((unsigned)x >= (1u << level) || (unsigned)y >= (1u << level) || (unsigned)z >= (1u << level)) continue;
      const uint32_t e = d.tab[tab_index(d, level, x, y, z)];
      if (e == 0u || e == SE_PENDING) continue;
      nid = e - 1u;
    }
    const uint32_t si = min(a.nsrc[i >> 3], a.nn - 1u);
    const size_t va = (size_t)nid * 8 + (i & 7), vb = (size_t)si * 8 + (i & 7);
    float vx = d.nx[va], vy = d.ny[va];
    se_merge_value<OFUSION>(vx, vy, m.nx[vb], m.ny[vb], mode, maxw, ix, iy);
    d.nx[va] = vx; d.ny[va] = vy;
  }
}
