// Release of map regions and of blocks that hold nothing (se_hip_release_boxes, include/se_hip.h): octants wholly inside a record's box are handed
// back, all of them (SE_HIP_RELEASE_ALL) or only those that hold nothing (SE_HIP_RELEASE_UNSEEN).  The host restatement is
// include/se/release_map.hpp.
//
// It is the shift's route (se_shift_kernels.h) with s = 0 and another survival rule: the rule needs the content of every brick and the tree above it,
// the rest -- gather through staging, the index cleared, k_alloc_commit, scatter -- is the shift's own code.  Nothing here writes the map: the host
// reads the counts first, and a call that releases nothing leaves everything as it is.
//   k_release_blocks      a wave per block-list entry: the 4 KiB brick read raw, 16 bytes per lane and access as k_shift_gather reads it, reduced to "all
//                         initValue()" with one ballot; the records tested for containment 64 per step, a lane per record; the decision goes to a flag
//                         per brick slot, and a surviving block marks its ancestors in a per-node byte array by walking tab[] upwards (plain stores of 1)
//   k_release_nodes_mark  a lane per node: a node that is not releasable marks itself and its ancestors -- so an unmarked node is releasable and has
//                         no survivor beneath it: released
//   k_release_select      a lane per block and per node: the survivors compacted with se_wave_take into the key lists of ShiftArgs, in the form
//                         k_shift_select leaves them; a surviving node's value_[8] go to the staging with the entries above released octants already
//                         initValue(); the released blocks and nodes, the blocks that held something and the touched box are reduced per wave
//   k_release_root        (only when something is released) the same entry rule for the root, in place: it is not listed, it always exists
#pragma once
#include "se_merge_kernels.h"
#include "se_shift_kernels.h"

#define SE_RELEASE_ALL 1
#define SE_RELEASE_UNSEEN 2
#define SE_RELEASE_GONE 1u     // brel[]: released
#define SE_RELEASE_HELD 2u     // brel[]: ... and held at least one observed voxel

struct ReleaseRec { int lo[3]; int hi[3]; int what; int reserved; };   // hi = lo + side (the host adds: both within [-2^30, 2^30])

struct ReleaseArgs {
  ShiftArgs sh;                  // s = 0: the lists, the staging bricks and node values the shift's tail works on
  const ReleaseRec* rec;         // [n]
  uint32_t n;
  uint32_t nslots;               // brick slots of the map (pooled: the pool; dense: the cells of the block grid)
  uint8_t* brel;                 // [nslots] per brick slot, as the leaf entries of tab[] name a block: 0 stays, SE_RELEASE_GONE (| SE_RELEASE_HELD);
                                 // only the slots of existing blocks are written, and only those are read
  uint8_t* nstay;                // [nn] per node: 1 = it stays (zeroed before k_release_blocks; the root's is set by the host)
  uint32_t* cnt;                 // blocks released, nodes released, released blocks that held something
  int* box;                      // lo[3] (start: INT_MAX), hi[3] (start: INT_MIN): voxel corners of the released blocks, min and max + 8
};

// off[l] of DevMap as arithmetic (8 + 64 + ... + 8^(l-1)): l is a per-lane value here, and indexing the by-value array with it would put it in scratch
__device__ __forceinline__ uint32_t se_release_tab(const DevMap& m, int l, int x, int y, int z) {
  return (((1u << (3 * l)) - 8u) / 7u) + (((((uint32_t)z << l) | (uint32_t)y) << l) | (uint32_t)x);
}
// the node with position (x, y, z) at level l >= 1 and every ancestor of it below the root is marked as staying
__device__ __forceinline__ void se_release_mark_up(const DevMap& m, const ReleaseArgs& a, int l, int x, int y, int z) {
  for (; l >= 1; --l, x >>= 1, y >>= 1, z >>= 1) {
    const uint32_t e = m.tab[se_release_tab(m, l, x, y, z)];
    if (e != 0u && e != SE_PENDING && e - 1u < a.sh.nn) a.nstay[e - 1u] = 1;
  }
}
// does a record contain the octant with voxel corner (x, y, z) and side d?
__device__ __forceinline__ bool se_release_contains(const ReleaseRec& r, int x, int y, int z, int d) {
  return x >= r.lo[0] && y >= r.lo[1] && z >= r.lo[2] && x + d <= r.hi[0] && y + d <= r.hi[1] && z + d <= r.hi[2];
}

__global__ __launch_bounds__(SE_WG) void k_release_blocks(DevMap m, ReleaseArgs a) {
  const uint32_t lane = threadIdx.x & 63u, nwaves = gridDim.x * (SE_WG / 64);
  const uint32_t ix = __float_as_uint(m.init_x);
  // the y plane of the pattern k_fill_bricks leaves: floats of initValue().y, or (SDF) the weight bytes, the first 512 bytes of the plane
  const uint32_t iy = m.ybyte ? (uint32_t)(uint8_t)(int)m.init_y * 0x01010101u : __float_as_uint(m.init_y);
  for (uint32_t b = blockIdx.x * (SE_WG / 64) + (threadIdx.x >> 6); b < a.sh.nb; b += nwaves) {
    const uint32_t bp = m.bpos[b];
    const uint32_t slot = block_slot(m, b, bp);
    const uint4* src = (const uint4*)(m.vx + (size_t)slot * SE_BRICK_STRIDE);
    const uint4 v0 = src[lane], v1 = src[lane + 64];
    bool differs = v0.x != ix || v0.y != ix || v0.z != ix || v0.w != ix || v1.x != ix || v1.y != ix || v1.z != ix || v1.w != ix;
    if (m.ybyte) {
      if (lane < 32u) { const uint4 w = src[lane + 128]; differs = differs || w.x != iy || w.y != iy || w.z != iy || w.w != iy; }
    } else {
      const uint4 w0 = src[lane + 128], w1 = src[lane + 192];
      differs = differs || w0.x != iy || w0.y != iy || w0.z != iy || w0.w != iy || w1.x != iy || w1.y != iy || w1.z != iy || w1.w != iy;
    }
    const bool empty = __ballot(differs) == 0ull;
    const int bx = (int)(bp & 1023u), by = (int)((bp >> 10) & 1023u), bz = (int)(bp >> 20);
    bool all = false, any = false;
    for (uint32_t r0 = 0; r0 < a.n && !all; r0 += 64u) {
      const uint32_t r = r0 + lane;
      bool in = false, whole = false;
      if (r < a.n) {
        const ReleaseRec rec = a.rec[r];
        in = se_release_contains(rec, bx * 8, by * 8, bz * 8, 8);
        whole = in && rec.what == SE_RELEASE_ALL;
      }
      any = any || __ballot(in) != 0ull;
      all = __ballot(whole) != 0ull;
    }
    const bool gone = all || (any && empty);
    if (lane == 0u) {
      a.brel[slot] = gone ? (uint8_t)(SE_RELEASE_GONE | (empty ? 0u : SE_RELEASE_HELD)) : (uint8_t)0;
      if (!gone) se_release_mark_up(m, a, m.leaf_level - 1, bx >> 1, by >> 1, bz >> 1);
    }
  }
}

__global__ __launch_bounds__(SE_WG) void k_release_nodes_mark(DevMap m, ReleaseArgs a) {
  for (uint32_t i = 1u + blockIdx.x * SE_WG + threadIdx.x; i < a.sh.nn; i += gridDim.x * SE_WG) {   // (node 0 is the root: it always stays)
    const int level = (int)m.nlevel[i];
    const uint32_t np = m.npos[i];
    const int sh = m.max_level - level;
    const int x = (int)(np & 1023u), y = (int)((np >> 10) & 1023u), z = (int)(np >> 20);
    bool empty = true;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      empty = empty && __float_as_uint(m.nx[(size_t)i * 8 + j]) == __float_as_uint(m.init_x) && __float_as_uint(m.ny[(size_t)i * 8 + j]) == __float_as_uint(m.init_y);
    bool all = false, any = false;
    for (uint32_t r = 0; r < a.n; ++r) {
      const ReleaseRec rec = a.rec[r];
      const bool in = se_release_contains(rec, x << sh, y << sh, z << sh, 1 << sh);
      any = any || in;
      all = all || (in && rec.what == SE_RELEASE_ALL);
    }
    if (!(all || (any && empty))) se_release_mark_up(m, a, level, x, y, z);
  }
}

// value_[j] of the surviving node (level, x, y, z): initValue() where the child octant exists and is released
__device__ __forceinline__ bool se_release_child_gone(const DevMap& m, const ReleaseArgs& a, int level, int x, int y, int z, int j) {
  const int cl = level + 1, cx = 2 * x + (j & 1), cy = 2 * y + ((j >> 1) & 1), cz = 2 * z + (j >> 2);
  const uint32_t e = m.tab[se_release_tab(m, cl, cx, cy, cz)];
  if (e == 0u || e == SE_PENDING) return false;
  if (cl == m.leaf_level) return e - 1u < a.nslots && a.brel[e - 1u] != 0;
  return e - 1u < a.sh.nn && a.nstay[e - 1u] == 0;
}

__global__ __launch_bounds__(SE_WG) void k_release_select(DevMap m, ReleaseArgs a) {
  const uint32_t n = max(a.sh.nb, a.sh.nn);
  const uint32_t rounds = (n + gridDim.x * SE_WG - 1) / (gridDim.x * SE_WG);   // every lane of a wave makes every round (ballots, shuffles)
  const uint32_t lane = threadIdx.x & 63u;
  for (uint32_t r = 0; r < rounds; ++r) {
    const uint32_t i = (r * gridDim.x + blockIdx.x) * SE_WG + threadIdx.x;
    {
      const bool is_block = i < a.sh.nb;
      const uint32_t bp = is_block ? m.bpos[i] : 0u;
      const uint32_t slot = block_slot(m, i, bp);
      const uint32_t flag = is_block ? (uint32_t)a.brel[slot] : 0u;
      const int x = (int)(bp & 1023u), y = (int)((bp >> 10) & 1023u), z = (int)(bp >> 20);
      const bool keep = is_block && flag == 0u, gone = is_block && flag != 0u;
      const unsigned long long at = se_wave_take(&a.sh.blist[0], keep);
      if (keep) {
        a.sh.blist[1 + at] = se_make_key(x, y, z, m.leaf_level, m.max_level);
        a.sh.bact[at] = m.bactive[slot];
      }
      if (is_block) a.sh.dst[i] = keep ? (uint32_t)at : SE_SHIFT_DROPPED;
      const unsigned long long gm = __ballot(gone);
      if (gm != 0ull) {
        const unsigned long long hm = __ballot(gone && (flag & SE_RELEASE_HELD) != 0u);
        const int big = 0x7FFFFFFF;
        const int lx = se_wave_min(gone ? x : big), ly = se_wave_min(gone ? y : big), lz = se_wave_min(gone ? z : big);
        const int hx = se_wave_max(gone ? x : -1), hy = se_wave_max(gone ? y : -1), hz = se_wave_max(gone ? z : -1);
        if (lane == 0u) {
          atomicAdd(&a.cnt[0], (uint32_t)__builtin_popcountll(gm));
          if (hm != 0ull) atomicAdd(&a.cnt[2], (uint32_t)__builtin_popcountll(hm));
          atomicMin(&a.box[0], lx * 8); atomicMin(&a.box[1], ly * 8); atomicMin(&a.box[2], lz * 8);
          atomicMax(&a.box[3], hx * 8 + 8); atomicMax(&a.box[4], hy * 8 + 8); atomicMax(&a.box[5], hz * 8 + 8);
        }
      }
    }
    {
      const bool is_node = i >= 1u && i < a.sh.nn;   // (the root is not listed: it always exists)
      const int level = is_node ? (int)m.nlevel[i] : 1;
      const uint32_t np = is_node ? m.npos[i] : 0u;
      const int x = (int)(np & 1023u), y = (int)((np >> 10) & 1023u), z = (int)(np >> 20);
      const bool keep = is_node && a.nstay[i] != 0, gone = is_node && !keep;
      const unsigned long long at = se_wave_take(&a.sh.nlist[0], keep);
      if (keep) {
        a.sh.nlist[1 + at] = se_make_key(x, y, z, level, m.max_level);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const bool reset = se_release_child_gone(m, a, level, x, y, z, j);
          a.sh.nval[at * 16 + j] = reset ? m.init_x : m.nx[(size_t)i * 8 + j];
          a.sh.nval[at * 16 + 8 + j] = reset ? m.init_y : m.ny[(size_t)i * 8 + j];
        }
      }
      const unsigned long long gm = __ballot(gone);
      if (gm != 0ull && lane == (uint32_t)__builtin_ctzll(gm)) atomicAdd(&a.cnt[1], (uint32_t)__builtin_popcountll(gm));
    }
  }
}

__global__ __launch_bounds__(64) void k_release_root(DevMap m, ReleaseArgs a) {
  const int j = (int)threadIdx.x;
  if (j < 8 && se_release_child_gone(m, a, 0, 0, 0, 0, j)) { m.nx[j] = m.init_x; m.ny[j] = m.init_y; }
}
