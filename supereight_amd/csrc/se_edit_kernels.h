// Batched axis-aligned region edits of the resident map (se_hip_edit_boxes, include/se_hip.h): the reference's
// se::functor::axis_aligned_map(map, f, min, max) (se_core/include/se/functors/axis_aligned_functor.hpp) for a list of boxes at once, f being
// "assign x and / or y where the current value has one of these classes".  Existing blocks and nodes only; values only -- nothing that
// the raycast or the scan derive from the map (tab[], occ[], lbits[], cbits[], fbits[], bpos[], bactive[]) is touched.
//
// List order without any order between waves: an edit is pointwise, so "the edits one after another" equals "every value walks the list in
// order and applies the edits that contain it".  A wave owns one block (k_edit_blocks: lane = column x + 8y, the eight z slices in registers)
// or eight nodes (k_edit_nodes: lane = node, child) for the whole list:
//   - 64 edits per step, one per lane: validity, flag and the wave-uniform overlap test (block against box) are evaluated lane-parallel, so
//     an edit that does not concern the wave costs 1 / 64 of a step;
//   - the survivors (ballot) are applied in ascending lane order = list order, their fields broadcast with readlane;
//   - a brick is read when the first surviving edit arrives and written back once, after the list, if a value changed: a block no valid
//     edit overlaps causes no brick traffic.
// Counts: one 64-bit vector atomic per wave and counter after a wave reduction.
#pragma once
#include "se_collide_kernels.h"

#define SE_EDIT_SET_X 1u
#define SE_EDIT_SET_Y 2u
#define SE_EDIT_BLOCKS 4u
#define SE_EDIT_NODES 8u
#define SE_EDIT_FLAGS 15u
#define SE_EDIT_LIMIT (1 << 30)   // every coordinate of lo and hi within [-2^30, 2^30], else the edit is invalid

struct EditRec { int32_t lo[3], hi[3]; float x, y; uint32_t flags, only; };   // se_hip_edit
static_assert(sizeof(EditRec) == 40, "se_hip_edit is 40 bytes");
// test_ok: the call's se_hip_collide_test is usable (non-null, finite threshold, occupied_above 0 / 1); counts: null = not wanted
struct EditArgs { const EditRec* edits; long long n; float thr; int above; int test_ok; int reference; unsigned long long* counts; };

// The rules of include/se_hip.h ("invalid edits"); reads the record only.
__device__ __forceinline__ bool se_edit_valid(const DevMap& m, const EditArgs& a, const EditRec& e) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    ok = ok && e.lo[k] >= -SE_EDIT_LIMIT && e.lo[k] <= SE_EDIT_LIMIT && e.hi[k] >= -SE_EDIT_LIMIT && e.hi[k] <= SE_EDIT_LIMIT;
  ok = ok && (e.flags & ~SE_EDIT_FLAGS) == 0u && e.only >= 1u && e.only <= 7u && (e.only == 7u || a.test_ok);
  if (e.flags & SE_EDIT_SET_X) ok = ok && isfinite(e.x);
  if (e.flags & SE_EDIT_SET_Y) {
    ok = ok && isfinite(e.y);
    if (m.ybyte) ok = ok && e.y >= 0.f && e.y <= 255.f && e.y == (float)(int)e.y;   // the weight lives in a byte
  }
  return ok;
}

// Edit i of the list for this lane (a zeroed record beyond the end), and whether it is valid.
__device__ __forceinline__ EditRec se_edit_load(const DevMap& m, const EditArgs& a, long long i, bool& valid) {
  EditRec e = {};
  valid = false;
  if (i < a.n) {
    e = a.edits[i];   // (ten 4-byte loads: the struct, and so a caller's array, is only 4-byte aligned)
    valid = se_edit_valid(m, a, e);
  }
  return e;
}

// the record of lane `w`, in every lane
__device__ __forceinline__ EditRec se_edit_bcast(const EditRec& e, int w) {
  EditRec r;
#pragma unroll
  for (int k = 0; k < 3; ++k) { r.lo[k] = __builtin_amdgcn_readlane(e.lo[k], w); r.hi[k] = __builtin_amdgcn_readlane(e.hi[k], w); }
  r.x = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(e.x), w));
  r.y = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(e.y), w));
  r.flags = (uint32_t)__builtin_amdgcn_readlane((int)e.flags, w);
  r.only = (uint32_t)__builtin_amdgcn_readlane((int)e.only, w);
  return r;
}

// sum over the wave, valid in lane 0
__device__ __forceinline__ unsigned long long se_edit_wave_sum(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
  return v;
}

// does the current value (x, y) have one of the classes of `only`?  (bit = 1 << class code of se_collide_class)
__device__ __forceinline__ bool se_edit_pred(uint32_t only, float x, float y, const FieldConst fc, float thr, int above) {
  return only == 7u || ((only >> se_collide_class(x, y, fc, thr, above)) & 1u) != 0u;
}

// One wave per entry of the block list (grid-stride).  counts[0] += voxel applications, counts[2] += blocks with one.
__global__ __launch_bounds__(SE_WG) void k_edit_blocks(DevMap m, EditArgs a) {
  const FieldConst fc = se_field_const(m);
  const int lane = (int)(threadIdx.x & 63u);
  const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * SE_WG + threadIdx.x) >> 6));
  const int nwaves = (int)((gridDim.x * SE_WG) >> 6);
  const uint32_t nblocks = min(m.ctr[C_BLOCKS], m.cap_blocks);
  for (uint32_t b = (uint32_t)wave; b < nblocks; b += (uint32_t)nwaves) {
    const uint32_t bp = (uint32_t)__builtin_amdgcn_readfirstlane((int)m.bpos[b]);
    const int bx = (int)(bp & 1023u) << 3, by = (int)((bp >> 10) & 1023u) << 3, bz = (int)(bp >> 20) << 3;
    const int x = bx + (lane & 7), y = by + (lane >> 3);
    float* brick = m.vx + (size_t)block_slot(m, b, bp) * SE_BRICK_STRIDE;
    float vx[8], vy[8];
    bool loaded = false, dirty = false;
    unsigned long long applied = 0ull;
    for (long long base = 0; base < a.n; base += 64) {
      bool valid;
      const EditRec mine = se_edit_load(m, a, base + lane, valid);
      const bool ov = valid && (mine.flags & SE_EDIT_BLOCKS) != 0u && mine.lo[0] < bx + 8 && mine.hi[0] > bx && mine.lo[1] < by + 8 && mine.hi[1] > by &&
                      mine.lo[2] < bz + 8 && mine.hi[2] > bz;
      unsigned long long todo = __ballot(ov);
      while (todo) {
        const int w = (int)__builtin_ctzll(todo);
        todo &= todo - 1ull;
        const EditRec e = se_edit_bcast(mine, w);
        if (!loaded) {   // slice z of the x plane is one coalesced row of 64 floats; the eight weights of an SDF column are one 8-byte word
          loaded = true;
#pragma unroll
          for (int z = 0; z < 8; ++z) vx[z] = brick[lane + 64 * z];
          if (m.ybyte) {
            const uint2 q = *(const uint2*)((const uint8_t*)(brick + 512) + 8 * lane);   // bytes SE_YB(lane + 64 z) = 8 lane + z
#pragma unroll
            for (int z = 0; z < 8; ++z) vy[z] = (float)(((z < 4 ? q.x : q.y) >> (8 * (z & 3))) & 255u);
          } else {
#pragma unroll
            for (int z = 0; z < 8; ++z) vy[z] = brick[512 + lane + 64 * z];
          }
        }
        const bool col = x >= e.lo[0] && x < e.hi[0] && y >= e.lo[1] && y < e.hi[1];
#pragma unroll
        for (int z = 0; z < 8; ++z) {
          if (col && bz + z >= e.lo[2] && bz + z < e.hi[2] && se_edit_pred(e.only, vx[z], vy[z], fc, a.thr, a.above)) {
            ++applied;
            if (e.flags & SE_EDIT_SET_X) { vx[z] = e.x; dirty = true; }
            if (e.flags & SE_EDIT_SET_Y) { vy[z] = e.y; dirty = true; }
          }
        }
      }
    }
    if (!loaded) continue;
    if (__ballot(dirty) != 0ull) {
#pragma unroll
      for (int z = 0; z < 8; ++z) brick[lane + 64 * z] = vx[z];
      if (m.ybyte) {
        uint2 q = {0u, 0u};
#pragma unroll
        for (int z = 0; z < 8; ++z) {
          const uint32_t byte = (uint32_t)(int)vy[z] << (8 * (z & 3));
          if (z < 4) q.x |= byte; else q.y |= byte;
        }
        *(uint2*)((uint8_t*)(brick + 512) + 8 * lane) = q;
      } else {
#pragma unroll
        for (int z = 0; z < 8; ++z) brick[512 + lane + 64 * z] = vy[z];
      }
    }
    if (a.counts) {
      const unsigned long long tot = se_edit_wave_sum(applied);
      if (lane == 0 && tot) { atomicAdd(&a.counts[0], tot); atomicAdd(&a.counts[2], 1ull); }
    }
  }
}

// One thread per (node, child) (grid-stride over waves of eight nodes): counts[1] += node-value applications.  The waves also count the
// invalid edits of the list, each edit once: counts[3].
__global__ __launch_bounds__(SE_WG) void k_edit_nodes(DevMap m, EditArgs a) {
  const FieldConst fc = se_field_const(m);
  const int lane = (int)(threadIdx.x & 63u);
  const long long wave = (long long)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * SE_WG + threadIdx.x) >> 6));
  const long long nwaves = (long long)((gridDim.x * SE_WG) >> 6);
  if (a.counts) {
    unsigned long long bad = 0ull;
    for (long long base = wave * 64; base < a.n; base += nwaves * 64) {
      bool valid;
      se_edit_load(m, a, base + lane, valid);
      bad += (base + lane < a.n && !valid) ? 1ull : 0ull;
    }
    bad = se_edit_wave_sum(bad);
    if (lane == 0 && bad) atomicAdd(&a.counts[3], bad);
  }
  const uint32_t nnodes = min(m.ctr[C_NODES], m.cap_nodes);
  const int child = lane & 7;
  // REFERENCE: the running sum of dir(i) * side / 2 over i = 0 .. child, in units of side / 2
  const int cum_x = (0x43322110 >> (4 * child)) & 15, cum_y = (0x43222100 >> (4 * child)) & 15, cum_z = (0x43210000 >> (4 * child)) & 15;
  for (long long n0 = wave * 8; n0 < (long long)nnodes; n0 += nwaves * 8) {
    const uint32_t node = (uint32_t)n0 + (uint32_t)(lane >> 3);
    const bool live = node < nnodes;
    int c[3] = {0, 0, 0}, t[3] = {0, 0, 0}, h = 0;
    float vx = 0.f, vy = 0.f;
    if (live) {
      const uint32_t np = m.npos[node];
      const int lvl = (int)m.nlevel[node];
      const int sh = m.max_level - lvl;
      h = (m.size >> lvl) >> 1;
      const int corner[3] = {(int)(np & 1023u) << sh, (int)((np >> 10) & 1023u) << sh, (int)(np >> 20) << sh};
      // STRICT: the child octant's corner.  REFERENCE: unpack_morton(code_ | level) -- the level's bits 0 and 3 land in x, 1 and 4 in y, 2 in z --
      // plus the cumulative offset
      c[0] = corner[0] + ((child & 1) ? h : 0); c[1] = corner[1] + ((child & 2) ? h : 0); c[2] = corner[2] + ((child & 4) ? h : 0);
      t[0] = corner[0] + ((lvl & 1) | (((lvl >> 3) & 1) << 1)) + cum_x * h;
      t[1] = corner[1] + (((lvl >> 1) & 1) | (((lvl >> 4) & 1) << 1)) + cum_y * h;
      t[2] = corner[2] + ((lvl >> 2) & 1) + cum_z * h;
      vx = m.nx[(size_t)node * 8 + child]; vy = m.ny[(size_t)node * 8 + child];
    }
    bool dirty = false;
    unsigned long long applied = 0ull;
    for (long long base = 0; base < a.n; base += 64) {
      bool valid;
      const EditRec mine = se_edit_load(m, a, base + lane, valid);
      unsigned long long todo = __ballot(valid && (mine.flags & SE_EDIT_NODES) != 0u);
      while (todo) {
        const int w = (int)__builtin_ctzll(todo);
        todo &= todo - 1ull;
        const EditRec e = se_edit_bcast(mine, w);
        bool in = live;
#pragma unroll
        for (int k = 0; k < 3; ++k)
          in = in && (a.reference ? (e.lo[k] <= t[k] && t[k] <= e.hi[k]) : (e.lo[k] <= c[k] && c[k] + h <= e.hi[k]));
        if (in && se_edit_pred(e.only, vx, vy, fc, a.thr, a.above)) {
          ++applied;
          if (e.flags & SE_EDIT_SET_X) { vx = e.x; dirty = true; }
          if (e.flags & SE_EDIT_SET_Y) { vy = e.y; dirty = true; }
        }
      }
    }
    if (dirty) { m.nx[(size_t)node * 8 + child] = vx; m.ny[(size_t)node * 8 + child] = vy; }
    if (a.counts) {
      const unsigned long long tot = se_edit_wave_sum(applied);
      if (lane == 0 && tot) atomicAdd(&a.counts[1], tot);
    }
  }
}
