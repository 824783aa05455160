// Shift of the resident map by whole blocks (se_hip_shift_map, include/se_hip.h): content at voxel c is at c + s afterwards, what leaves the cube is
// forgotten, the vacated side is unseen.  The host restatement is include/se/shift_map.hpp.
//
// Nothing is moved in place -- in a dense grid the new position of one brick is the old position of another, and no order of the bricks is free of
// that hazard without a second grid.  The survivors go through staging instead (4 KiB per surviving block), and the work is per block, not per cell:
//   k_shift_select   a lane per block-list entry and per node entry: survival, the new key; the survivors of a wave are compacted with se_wave_take
//                    (ballot, one atomic, mbcnt rank) into the two key lists of the staging; a surviving node's value_[8] goes there with it, and every
//                    node slot is rewritten with initValue()
//   k_shift_gather   a wave per OLD block: the 4 KiB slot copied raw (16 bytes per lane and access: the kernel knows nothing of the byte weights of
//                    SDF or of the OFusion planes), then the same slot rewritten with the init pattern and its active flag cleared -- a wave touches
//                    its own slot only; a dropped block is only reset
//   (host)           the index structures cleared, then the two key lists inserted by k_alloc_commit: tab[], occ[], lbits[], cbits[], fbits[], bpos[],
//                    npos[], nlevel[] and the counters are those of a map that was allocated that way, missing ancestors included
//   k_shift_scatter  a wave per survivor: the slot from tab[], the brick and bactive[] written; node values by key, as k_load_nodes does
#pragma once
#include "se_kernels.h"

#define SE_SHIFT_LIMIT (1 << 30)          // every component of the shift within [-2^30, 2^30]
#define SE_SHIFT_DROPPED 0xFFFFFFFFu

struct ShiftArgs {
  int s[3];                      // voxels, multiples of 8
  uint32_t nb, nn;               // blocks / nodes (root included) of the map before the call, never more than the pools hold
  uint4* bricks;                 // [nb] x 256: the surviving bricks, in the order of blist
  float* nval;                   // [nn] x 16: value_[8] of the surviving nodes, the 8 x then the 8 y, in the order of nlist
  unsigned long long* blist;     // [count, key ...]: the new keys of the surviving blocks
  unsigned long long* nlist;     // ... of the surviving nodes (the root is not listed: it always exists)
  uint32_t* dst;                 // [nb] per old list position: its place in blist, or SE_SHIFT_DROPPED
  uint8_t* bact;                 // [nb] VoxelBlock::active_ of the survivors, in the order of blist
};

__global__ __launch_bounds__(SE_WG) void k_shift_select(DevMap m, ShiftArgs a) {
  const uint32_t n = max(a.nb, a.nn);
  const uint32_t rounds = (n + gridDim.x * SE_WG - 1) / (gridDim.x * SE_WG);   // every lane of a wave makes every round (se_wave_take ballots)
  for (uint32_t r = 0; r < rounds; ++r) {
    const uint32_t i = (r * gridDim.x + blockIdx.x) * SE_WG + threadIdx.x;
    {
      // block i: its corner + s within [0, size - 8] on every axis
      const bool is_block = i < a.nb;
      const uint32_t bp = is_block ? m.bpos[i] : 0u;
      const int nblk = 1 << m.leaf_level;
      const int x = (int)(bp & 1023u) + (a.s[0] >> 3), y = (int)((bp >> 10) & 1023u) + (a.s[1] >> 3), z = (int)(bp >> 20) + (a.s[2] >> 3);
      const bool keep = is_block && (unsigned)x < (unsigned)nblk && (unsigned)y < (unsigned)nblk && (unsigned)z < (unsigned)nblk;
      const unsigned long long at = se_wave_take(&a.blist[0], keep);
      if (keep) {
        a.blist[1 + at] = se_make_key(x, y, z, m.leaf_level, m.max_level);
        a.bact[at] = m.bactive[block_slot(m, i, bp)];
      }
      if (is_block) a.dst[i] = keep ? (uint32_t)at : SE_SHIFT_DROPPED;
    }
    {
      // node i of side d: s a multiple of d on every axis and its corner + s within [0, size - d]; the root (i = 0, level 0) only gives up its values
      const bool is_node = i < a.nn;
      const int level = is_node ? (int)m.nlevel[i] : 0;
      const uint32_t np = is_node ? m.npos[i] : 0u;
      const int sh = m.max_level - level;
      const int low = (1 << sh) - 1;
      const bool aligned = ((a.s[0] | a.s[1] | a.s[2]) & low) == 0;
      const int x = (int)(np & 1023u) + (a.s[0] >> sh), y = (int)((np >> 10) & 1023u) + (a.s[1] >> sh), z = (int)(np >> 20) + (a.s[2] >> sh);
      const int cells = 1 << level;
      const bool keep = is_node && level >= 1 && level < m.leaf_level && aligned && (unsigned)x < (unsigned)cells && (unsigned)y < (unsigned)cells && (unsigned)z < (unsigned)cells;
      const unsigned long long at = se_wave_take(&a.nlist[0], keep);
      if (keep) a.nlist[1 + at] = se_make_key(x, y, z, level, m.max_level);
      if (is_node) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const size_t v = (size_t)i * 8 + j;
          if (keep) { a.nval[at * 16 + j] = m.nx[v]; a.nval[at * 16 + 8 + j] = m.ny[v]; }
          m.nx[v] = m.init_x; m.ny[v] = m.init_y;
        }
      }
    }
  }
}

__global__ __launch_bounds__(SE_WG) void k_shift_gather(DevMap m, ShiftArgs a) {
  const uint32_t lane = threadIdx.x & 63u, nwaves = gridDim.x * (SE_WG / 64);
  const uint4 ix = {__float_as_uint(m.init_x), __float_as_uint(m.init_x), __float_as_uint(m.init_x), __float_as_uint(m.init_x)};
  const uint4 iy = {__float_as_uint(m.init_y), __float_as_uint(m.init_y), __float_as_uint(m.init_y), __float_as_uint(m.init_y)};
  for (uint32_t b = blockIdx.x * (SE_WG / 64) + (threadIdx.x >> 6); b < a.nb; b += nwaves) {
    const uint32_t slot = block_slot(m, b, m.bpos[b]);
    const uint32_t d = a.dst[b];
    uint4* src = (uint4*)(m.vx + (size_t)slot * SE_BRICK_STRIDE);
    if (d != SE_SHIFT_DROPPED) {
      uint4* out = a.bricks + (size_t)d * 256;
      const uint4 v0 = src[lane], v1 = src[lane + 64], v2 = src[lane + 128], v3 = src[lane + 192];
      out[lane] = v0; out[lane + 64] = v1; out[lane + 128] = v2; out[lane + 192] = v3;
    }
    // the pattern k_fill_bricks leaves: 512 floats of initValue().x, 512 of initValue().y (SDF byte weights: 0 in every byte)
    src[lane] = ix; src[lane + 64] = ix; src[lane + 128] = iy; src[lane + 192] = iy;
    if (lane == 0) m.bactive[slot] = 0;
  }
}

__global__ __launch_bounds__(SE_WG) void k_shift_scatter(DevMap m, ShiftArgs a) {
  const uint32_t lane = threadIdx.x & 63u, nwaves = gridDim.x * (SE_WG / 64);
  const uint32_t kept = (uint32_t)min(a.blist[0], (unsigned long long)a.nb);
  const int bsh = m.max_level - m.leaf_level;
  for (uint32_t i = blockIdx.x * (SE_WG / 64) + (threadIdx.x >> 6); i < kept; i += nwaves) {
    const unsigned long long code = a.blist[1 + i] & ~0x1FFull;
    const int x = (int)(se_compact21(code) >> bsh), y = (int)(se_compact21(code >> 1) >> bsh), z = (int)(se_compact21(code >> 2) >> bsh);
    const uint32_t e = m.tab[leaf_index(m, x, y, z)];
    if (e == 0u || e == SE_PENDING) continue;   // (the pool ran out while the list was inserted: reported by the call)
    const uint4* in = a.bricks + (size_t)i * 256;
    uint4* out = (uint4*)(m.vx + (size_t)(e - 1u) * SE_BRICK_STRIDE);
    const uint4 v0 = in[lane], v1 = in[lane + 64], v2 = in[lane + 128], v3 = in[lane + 192];
    out[lane] = v0; out[lane + 64] = v1; out[lane + 128] = v2; out[lane + 192] = v3;
    if (lane == 0) m.bactive[e - 1u] = a.bact[i];
  }
  const unsigned long long nkept = min(a.nlist[0], (unsigned long long)a.nn);
  for (unsigned long long i = blockIdx.x * (unsigned long long)SE_WG + threadIdx.x; i < nkept * 8; i += (unsigned long long)gridDim.x * SE_WG) {
    const unsigned long long key = a.nlist[1 + (i >> 3)];
    const int level = (int)(key & 0x1FFull);
    const unsigned long long code = key & ~0x1FFull;
    const int sh = m.max_level - level;
    const int x = (int)(se_compact21(code) >> sh), y = (int)(se_compact21(code >> 1) >> sh), z = (int)(se_compact21(code >> 2) >> sh);
    const uint32_t e = m.tab[tab_index(m, level, x, y, z)];
    if (e == 0u || e == SE_PENDING) continue;
    m.nx[(size_t)(e - 1u) * 8 + (i & 7)] = a.nval[(i >> 3) * 16 + (i & 7)];
    m.ny[(size_t)(e - 1u) * 8 + (i & 7)] = a.nval[(i >> 3) * 16 + 8 + (i & 7)];
  }
}
