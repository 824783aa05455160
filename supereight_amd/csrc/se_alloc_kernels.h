// Batched region allocation of the resident map (se_hip_allocate_boxes, include/se_hip.h): Octree::allocate(key_t*, int)
// (se_core/include/se/octree.hpp:792-856) over the keys of every octant of a level that a list of voxel boxes touches -- without the keys[0] rule of
// unique_multiscale (k_zero_chain restates that rule for the OFusion scan; this entry does not apply it).  The host restatement is
// include/se/allocate_region.hpp.
//
// Box-driven, one launch for any list: the work is the sequence of CHUNKS -- 64 consecutive cells of a box's clipped octant range, x fastest -- of all
// boxes in list order, and wave w of W takes the chunks whose running number is w mod W.  Every wave walks the list 64 records per step, one per lane:
// validity, clipping and the chunk count are evaluated lane-parallel, a prefix sum over the lanes gives every box its first chunk number, and one
// subtraction tells the lane whether -- and where -- this wave has a chunk in its box.  So a box that does not concern the wave costs 1 / 64 of a
// step (thousands of small boxes), and one whole-volume box (32 768 chunks at 1024^3) is dealt evenly over the launch.
//   A chunk: a lane decodes its cell, asks lbits[] (leaf requests: "a block is allocated here", L2-resident) and goes to tab[] only where that bit is
// clear (coarse requests: tab[] directly); the lanes that found the entry empty call se_insert_octant with want = true, the others accompany the wave
// (it ballots and hands out pool slots with se_wave_take).  The caller passes the map with defer_occ = defer_mark = 0: occ[], lbits[], cbits[] and
// fbits[] are complete when the launch ends -- no raycast runs beside it (stream order), and the next one needs no commit pass.
//   Boxes may overlap and repeat: the compare-and-swap on the index entry elects one creator per octant, so the result is the union whatever the order.
// Counts: blocks / nodes created = the pool counters behind the launch minus in front of it (k_alloc_boxes_begin / _end: insertions by ancestors
// included); requested cells and invalid boxes are summed by wave 0, which sees the whole list like every wave.
#pragma once
#include "se_kernels.h"

#define SE_ALLOC_LIMIT (1 << 30)   // every coordinate of lo and hi within [-2^30, 2^30], else the box is invalid

struct AllocBox { int32_t lo[3], hi[3]; int32_t level; uint32_t reserved; };   // se_hip_alloc_box
static_assert(sizeof(AllocBox) == 32, "se_hip_alloc_box is 32 bytes");
// counts: null = not wanted; keys: [count, key ...] of the octants created at a requested level, null = not wanted; cap_keys = keys that fit behind the count
struct AllocBoxArgs { const AllocBox* boxes; long long n; unsigned long long* counts; unsigned long long* keys; unsigned long long cap_keys; };

// The box of this lane: its tree level, the corner and the extent of its clipped octant range (in octants of that level) and the number of cells
// (0: invalid, empty, inverted or wholly outside the volume).  Reads the record only.
struct AllocRange { int level; int lo[3]; uint32_t ex, ey; uint32_t cells; bool valid; };
__device__ __forceinline__ AllocRange se_alloc_range(const DevMap& m, const AllocBox& b) {
  AllocRange r = {};
  bool ok = b.reserved == 0u && b.level >= 0 && b.level <= m.leaf_level;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    ok = ok && b.lo[k] >= -SE_ALLOC_LIMIT && b.lo[k] <= SE_ALLOC_LIMIT && b.hi[k] >= -SE_ALLOC_LIMIT && b.hi[k] <= SE_ALLOC_LIMIT;
  r.valid = ok;
  r.level = (ok && b.level != 0) ? b.level : m.leaf_level;
  const int sh = m.max_level - r.level;
  uint32_t ext[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int lo = max(b.lo[k], 0), hi = min(b.hi[k], m.size);
    ok = ok && lo < hi;
    r.lo[k] = lo >> sh;
    ext[k] = ok ? (uint32_t)(((hi - 1) >> sh) - (lo >> sh) + 1) : 0u;
  }
  r.ex = ext[0]; r.ey = ext[1];
  r.cells = ok ? ext[0] * ext[1] * ext[2] : 0u;   // <= 8^leaf_level
  return r;
}

__global__ void k_alloc_boxes_begin(DevMap m, AllocBoxArgs a) {
  if (threadIdx.x != 0) return;
  if (a.counts) {
    a.counts[0] = 0ull - (unsigned long long)min(m.ctr[C_BLOCKS], m.cap_blocks);
    a.counts[1] = 0ull - (unsigned long long)min(m.ctr[C_NODES], m.cap_nodes);
    a.counts[2] = 0ull; a.counts[3] = 0ull;
  }
  if (a.keys) a.keys[0] = 0ull;
}
__global__ void k_alloc_boxes_end(DevMap m, AllocBoxArgs a) {
  if (threadIdx.x != 0 || !a.counts) return;
  a.counts[0] += (unsigned long long)min(m.ctr[C_BLOCKS], m.cap_blocks);
  a.counts[1] += (unsigned long long)min(m.ctr[C_NODES], m.cap_nodes);
}

__global__ __launch_bounds__(SE_WG) void k_alloc_boxes(DevMap m, AllocBoxArgs a) {
  const int lane = (int)(threadIdx.x & 63u);
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * SE_WG + threadIdx.x) >> 6));
  const uint32_t nwaves = (uint32_t)((gridDim.x * SE_WG) >> 6);
  uint32_t base = 0u;   // chunks of the boxes in front of this step, mod nwaves
  unsigned long long pairs = 0ull, bad = 0ull;
  for (long long b0 = 0; b0 < a.n; b0 += 64) {
    const bool in = b0 + lane < a.n;
    AllocBox box = {};
    if (in) box = a.boxes[b0 + lane];
    AllocRange r = se_alloc_range(m, box);
    if (!in) { r.cells = 0u; r.valid = true; }
    pairs += r.cells;
    bad += r.valid ? 0ull : 1ull;
    const uint32_t chunks = (r.cells + 63u) >> 6;
    uint32_t pre = chunks;   // inclusive prefix sum over the lanes: <= 64 * 8^leaf_level / 64
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(pre, d, 64); if (lane >= d) pre += t; }
    const uint32_t first = (base + (pre - chunks)) % nwaves;              // number of this box's chunk 0, mod nwaves
    const uint32_t mine = (wave + nwaves - first) % nwaves;               // this wave's first chunk in the box ...
    unsigned long long todo = __ballot(mine < chunks);                    // ... if the box has that many
    base = (base + (uint32_t)__builtin_amdgcn_readlane((int)pre, 63)) % nwaves;
    while (todo) {
      const int w = (int)__builtin_ctzll(todo);
      todo &= todo - 1ull;
      const int level = __builtin_amdgcn_readlane(r.level, w);
      const int ox = __builtin_amdgcn_readlane(r.lo[0], w), oy = __builtin_amdgcn_readlane(r.lo[1], w), oz = __builtin_amdgcn_readlane(r.lo[2], w);
      const uint32_t ex = (uint32_t)__builtin_amdgcn_readlane((int)r.ex, w), ey = (uint32_t)__builtin_amdgcn_readlane((int)r.ey, w);
      const uint32_t cells = (uint32_t)__builtin_amdgcn_readlane((int)r.cells, w);
      const uint32_t nchunks = (uint32_t)__builtin_amdgcn_readlane((int)chunks, w);
      const bool leaf = level == m.leaf_level;
      for (uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)mine, w); c < nchunks; c += nwaves) {
        const uint32_t cell = c * 64u + (uint32_t)lane;
        const bool live = cell < cells;
        const uint32_t i = live ? cell : 0u, t = i / ex;
        const int x = ox + (int)(i - t * ex), y = oy + (int)(t % ey), z = oz + (int)(t / ey);   // inside the level's grid: the range is clipped
        bool want = false;
        if (live) {
          if (leaf) {
            const uint32_t lin = block_linear(m, x, y, z);
            if (!((m.lbits[lin >> 5] >> (lin & 31u)) & 1u)) want = m.tab[m.leaf_off + lin] == 0u;
          } else {
            want = m.tab[tab_index(m, level, x, y, z)] == 0u;
          }
        }
        const bool made = se_insert_octant(m, level, x, y, z, want);
        if (a.keys && __ballot(made) != 0ull) {
          const unsigned long long at = se_wave_take(&a.keys[0], made);
          if (made && at < a.cap_keys) a.keys[1 + at] = se_make_key(x, y, z, level, m.max_level);
        }
      }
    }
  }
  if (a.counts && wave == 0u) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { pairs += __shfl_down(pairs, d, 64); bad += __shfl_down(bad, d, 64); }
    if (lane == 0) { a.counts[2] = pairs; a.counts[3] = bad; }
  }
}
