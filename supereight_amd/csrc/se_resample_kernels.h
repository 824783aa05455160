// Merge of one resident map into another under a rigid transform (se_hip_merge_map_rigid, include/se_hip.h): every destination voxel v reads the
// source field at q = R v + t (the pull transform, voxel units), blended from the eight voxels around q, and is combined with se_merge_value
// (se_merge_kernels.h).  The host restatement is se::rigid_sample / se::merge_map_rigid of include/se/merge_rigid.hpp.  One kernel holds both maps;
// the source is only read.
//   k_rigid_candidates  a lane per source block-list entry: the block's cube [c, c + 8]^3 carried into the destination by the inverse transform (double),
//                       its axis-aligned bounding box grown by one voxel and clipped to the volume; the destination blocks the box touches get their bit
//                       in a bitmap over the destination's block grid (block_linear order).  A superset: a valid sample's lower corner voxel is observed,
//                       so it lies in an allocated source block, and v lies in that block's pre-image (the voxel of margin takes the rounding of q)
//   k_rigid_list        a lane per bitmap word: the set bits become a list of packed block positions (one atomic per non-zero word)
//   k_rigid_eval        a wave per candidate block, lane = column (x, y), eight z per lane: does any voxel of the block get an observed sample?  The
//                       block's key goes into a key list (one atomic per participating wave); the destination voxel box is reduced per wave
//   (host)              k_alloc_commit on the destination over the key list: absent blocks are created with all ancestors, as the merge does
//   k_rigid_write       a wave per participating block: the samples again (recomputed: 4 KiB of staging per candidate block would be gigabytes at
//                       1024^3), se_merge_value, the brick stored back; SDF weights as ONE 8-byte access per lane; lane 0 sets bactive[]
// The sample (se_rigid_sample): the entries of the 4 x 4 x 4 source blocks around the block's image are loaded once per wave, one per lane, into LDS
// (the image of a block's lattice plus the upper corners spans at most 3 source blocks per axis); a corner's entry is an LDS read instead of a tab[]
// load.  A corner outside that neighbourhood (it cannot be, by the bound) is looked up in tab[], so the bound is not load-bearing.  A wave whose 64
// entries are all zero is done.  Non-finite source values: the result is unspecified (the library never produces them).
#pragma once
#include "se_merge_kernels.h"

struct RigidArgs {
  float pull[12];                // src_from_dst, row-major 3 x 4, voxels: q = R v + t
  double push[12];               // its inverse (candidates only)
  int mode;                      // SE_MERGE_*
  float max_weight;
  uint32_t nb;                   // blocks of the source
  uint32_t cap;                  // entries that cand[] and blist[] hold
  uint32_t words;                // words of cbm[]
  uint32_t* cbm;                 // candidate bitmap over the destination's block grid
  uint32_t* cand;                // [count, packed block position ...]
  unsigned long long* blist;     // [count, key ...]: destination keys of the participating blocks
  unsigned long long* nvox;      // [0] voxels with an observed sample, [1] of those, the destination voxel was observed before
  int* box;                      // lo[3] (start: INT_MAX), hi[3] (start: INT_MIN) over the participating blocks, voxels
};

// (The two small kernels are templates for the code object's sake only: hipcc emits plain kernels in the order of the translation unit and template
// instantiations behind them, so a plain kernel added here moves every per-frame kernel -- all of them templates -- to another address.)
template <int UNUSED>
__global__ __launch_bounds__(SE_WG) void k_rigid_candidates(DevMap d, DevMap m, RigidArgs a) {
  const int l = d.leaf_level;
  const double top = (double)(d.size - 1);
  for (uint32_t i = blockIdx.x * SE_WG + threadIdx.x; i < a.nb; i += gridDim.x * SE_WG) {
    const uint32_t bp = m.bpos[i];
    const double c[3] = {8.0 * (double)(bp & 1023u), 8.0 * (double)((bp >> 10) & 1023u), 8.0 * (double)(bp >> 20)};
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const double px = c[0] + ((k & 1) ? 8.0 : 0.0), py = c[1] + ((k & 2) ? 8.0 : 0.0), pz = c[2] + ((k & 4) ? 8.0 : 0.0);
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double w = ((a.push[4 * r] * px + a.push[4 * r + 1] * py) + a.push[4 * r + 2] * pz) + a.push[4 * r + 3];
        lo[r] = fmin(lo[r], w); hi[r] = fmax(hi[r], w);
      }
    }
    int b0[3], b1[3];
    bool any = true;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const double f = fmax(floor(lo[r]) - 1.0, 0.0), t = fmin(ceil(hi[r]) + 1.0, top);
      any = any && f <= t;
      b0[r] = any ? (int)f >> 3 : 0; b1[r] = any ? (int)t >> 3 : -1;
    }
    if (!any) continue;
    for (int z = b0[2]; z <= b1[2]; ++z)
      for (int y = b0[1]; y <= b1[1]; ++y)
        for (int x = b0[0]; x <= b1[0]; ++x) {
          const uint32_t idx = ((((uint32_t)z << l) | (uint32_t)y) << l) | (uint32_t)x;
          if ((idx >> 5) < a.words) atomicOr(&a.cbm[idx >> 5], 1u << (idx & 31u));
        }
  }
}

template <int UNUSED>
__global__ __launch_bounds__(SE_WG) void k_rigid_list(DevMap d, RigidArgs a) {
  const int l = d.leaf_level;
  const uint32_t mask = (1u << l) - 1u;
  for (uint32_t i = blockIdx.x * SE_WG + threadIdx.x; i < a.words; i += gridDim.x * SE_WG) {
    uint32_t w = a.cbm[i];
    if (w == 0u) continue;
    uint32_t at = atomicAdd(&a.cand[0], (uint32_t)__builtin_popcount(w));
    while (w) {
      const uint32_t idx = i * 32u + (uint32_t)__builtin_ctz(w);
      w &= w - 1u;
      if (at < a.cap) a.cand[1 + at] = pack_pos((int)(idx & mask), (int)((idx >> l) & mask), (int)(idx >> (2 * l)));
      ++at;
    }
  }
}

// q of the destination voxel (x, y, z): binary32, in the order of the definition
__device__ __forceinline__ float se_rigid_q(const RigidArgs& a, int r, float x, float y, float z) {
  return ((a.pull[4 * r] * x + a.pull[4 * r + 1] * y) + a.pull[4 * r + 2] * z) + a.pull[4 * r + 3];
}

// The wave's view of the source around the image of destination block (bx, by, bz): nbh[64] (LDS, this wave's) takes the entries of the 4 x 4 x 4
// source blocks from `base` on.  Returns false if the block cannot receive a sample (all 64 entries zero and the neighbourhood covers the image).
__device__ __forceinline__ bool se_rigid_neighbourhood(const DevMap& m, const RigidArgs& a, int bx, int by, int bz, uint32_t lane, uint32_t* nbh, int (&base)[3]) {
  float lo[3], hi[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) { lo[r] = 3.0e38f; hi[r] = -3.0e38f; }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float x = (float)(8 * bx + ((k & 1) ? 7 : 0)), y = (float)(8 * by + ((k & 2) ? 7 : 0)), z = (float)(8 * bz + ((k & 4) ? 7 : 0));
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const float q = se_rigid_q(a, r, x, y, z);
      lo[r] = fminf(lo[r], q); hi[r] = fmaxf(hi[r], q);
    }
  }
  // half a voxel either way takes the rounding of q between the lattice's corners (|q| <= 2^21: at most 0.25)
  bool covers = true;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int f = (int)floorf(lo[r] - 0.5f), t = (int)floorf(hi[r] + 0.5f) + 1;
    base[r] = f >> 3;
    covers = covers && (t >> 3) - base[r] <= 3;
  }
  const uint32_t e = se_query_block(m, base[0] + (int)(lane & 3u), base[1] + (int)((lane >> 2) & 3u), base[2] + (int)(lane >> 4));
  __builtin_amdgcn_wave_barrier();       // (the reads of the previous block are done)
  nbh[lane] = e;
  __builtin_amdgcn_wave_barrier();
  return __ballot(e != 0u) != 0ull || !covers;
}

// The sample at destination voxel (x, y, z): true iff valid, then (sx, sy) = b.  The caller tests b against initValue() for "observed".
template <bool OFUSION>
__device__ __forceinline__ bool se_rigid_sample(const DevMap& m, const RigidArgs& a, const uint32_t* nbh, const int (&base)[3], int x, int y, int z,
                                                float ix, float iy, float& sx, float& sy) {
  const float fx = (float)x, fy = (float)y, fz = (float)z;
  const float q0 = se_rigid_q(a, 0, fx, fy, fz), q1 = se_rigid_q(a, 1, fx, fy, fz), q2 = se_rigid_q(a, 2, fx, fy, fz);
  const float l0 = floorf(q0), l1 = floorf(q1), l2 = floorf(q2);
  const float top = (float)(m.size - 2);
  if (!(l0 >= 0.f && l0 <= top && l1 >= 0.f && l1 <= top && l2 >= 0.f && l2 <= top)) return false;
  const int cx = (int)l0, cy = (int)l1, cz = (int)l2;
  float p[8];
  float w = OFUSION ? -3.0e38f : 3.0e38f;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int vx = cx + (k & 1), vy = cy + ((k >> 1) & 1), vz = cz + (k >> 2);
    const int rx = (vx >> 3) - base[0], ry = (vy >> 3) - base[1], rz = (vz >> 3) - base[2];
    uint32_t e;
    if ((unsigned)rx < 4u && (unsigned)ry < 4u && (unsigned)rz < 4u) e = nbh[rx + 4 * ry + 16 * rz];
    else e = se_query_block(m, vx >> 3, vy >> 3, vz >> 3);
    const uint32_t v = (uint32_t)((vx & 7) + ((vy & 7) << 3) + ((vz & 7) << 6));
    const float* __restrict__ brick = m.vx + (size_t)(e ? e - 1u : 0u) * SE_BRICK_STRIDE;
    float px = ix, py = iy;
    if (e) {
      px = brick[v];
      py = OFUSION ? brick[512 + v] : (float)((const uint8_t*)(brick + 512))[SE_YB(v)];
    }
    ok = ok && !(px == ix && py == iy);
    p[k] = px;
    w = OFUSION ? fmaxf(w, py) : fminf(w, py);
  }
  if (!ok) return false;
  sx = se_trilerp(p, q0 - l0, q1 - l1, q2 - l2);
  sy = w;
  return true;
}

template <bool OFUSION>
__global__ __launch_bounds__(SE_WG) void k_rigid_eval(DevMap d, DevMap m, RigidArgs a) {
  __shared__ uint32_t s_nbh[SE_WG / 64][64];
  const uint32_t lane = threadIdx.x & 63u, nwaves = gridDim.x * (SE_WG / 64);
  uint32_t* nbh = s_nbh[threadIdx.x >> 6];
  const uint32_t ncand = min(a.cand[0], a.cap);
  const float ix = m.init_x, iy = m.init_y;
  const int big = 0x7FFFFFFF;
  int blo[3] = {big, big, big}, bhi[3] = {-1, -1, -1};      // (wave-uniform, in blocks)
  for (uint32_t i = blockIdx.x * (SE_WG / 64) + (threadIdx.x >> 6); i < ncand; i += nwaves) {
    const uint32_t bp = a.cand[1 + i];
    const int bx = (int)(bp & 1023u), by = (int)((bp >> 10) & 1023u), bz = (int)(bp >> 20);
    int base[3];
    if (!se_rigid_neighbourhood(m, a, bx, by, bz, lane, nbh, base)) continue;
    const int x = 8 * bx + (int)(lane & 7u), y = 8 * by + (int)(lane >> 3);
    bool seen = false;
    for (int k = 0; k < 8 && !seen; ++k) {
      float sx, sy;
      seen = se_rigid_sample<OFUSION>(m, a, nbh, base, x, y, 8 * bz + k, ix, iy, sx, sy) && !(sx == ix && sy == iy);
    }
    if (__ballot(seen) == 0ull) continue;
    if (lane == 0u) {
      const unsigned long long at = atomicAdd(&a.blist[0], 1ull);
      if (at < (unsigned long long)a.cap) a.blist[1 + at] = se_make_key(bx, by, bz, d.leaf_level, d.max_level);
    }
    blo[0] = min(blo[0], bx); blo[1] = min(blo[1], by); blo[2] = min(blo[2], bz);
    bhi[0] = max(bhi[0], bx); bhi[1] = max(bhi[1], by); bhi[2] = max(bhi[2], bz);
  }
  if (lane == 0u && bhi[0] >= 0) {
#pragma unroll
    for (int r = 0; r < 3; ++r) { atomicMin(&a.box[r], blo[r] * 8); atomicMax(&a.box[3 + r], bhi[r] * 8 + 8); }
  }
}

template <bool OFUSION>
__global__ __launch_bounds__(SE_WG) void k_rigid_write(DevMap d, DevMap m, RigidArgs a) {
  __shared__ uint32_t s_nbh[SE_WG / 64][64];
  const uint32_t lane = threadIdx.x & 63u, nwaves = gridDim.x * (SE_WG / 64);
  uint32_t* nbh = s_nbh[threadIdx.x >> 6];
  const uint32_t kept = (uint32_t)min(a.blist[0], (unsigned long long)a.cap);
  const int bsh = d.max_level - d.leaf_level;
  const int mode = a.mode;
  const float maxw = a.max_weight, ix = d.init_x, iy = d.init_y;
  uint32_t nobs = 0u, nboth = 0u;       // (per lane; summed over the wave at the end)
  for (uint32_t i = blockIdx.x * (SE_WG / 64) + (threadIdx.x >> 6); i < kept; i += nwaves) {
    const unsigned long long code = a.blist[1 + i] & ~0x1FFull;
    const int bx = (int)(se_compact21(code) >> bsh), by = (int)(se_compact21(code >> 1) >> bsh), bz = (int)(se_compact21(code >> 2) >> bsh);
    if ((unsigned)bx >= (1u << d.leaf_level) || (unsigned)by >= (1u << d.leaf_level) || (unsigned)bz >= (1u << d.leaf_level)) continue;
    const uint32_t e = d.tab[leaf_index(d, bx, by, bz)];
    if (e == 0u || e == SE_PENDING) continue;   // (the pool ran out while the list was inserted: reported by the call)
    int base[3];
    se_rigid_neighbourhood(m, a, bx, by, bz, lane, nbh, base);
    float* __restrict__ pa = d.vx + (size_t)(e - 1u) * SE_BRICK_STRIDE;
    const int x = 8 * bx + (int)(lane & 7u), y = 8 * by + (int)(lane >> 3);
    uint2 wa = {0u, 0u};
    if (!OFUSION) wa = ((const uint2*)(pa + 512))[lane];
    unsigned long long wb = ((unsigned long long)wa.y << 32) | wa.x;
    for (int k = 0; k < 8; ++k) {
      float sx, sy;
      if (!se_rigid_sample<OFUSION>(m, a, nbh, base, x, y, 8 * bz + k, ix, iy, sx, sy)) continue;
      if (sx == ix && sy == iy) continue;
      float ax = pa[lane + 64 * k];
      float ay = OFUSION ? pa[512 + lane + 64 * k] : (float)((wb >> (8 * k)) & 0xFFull);
      ++nobs;
      if (!(ax == ix && ay == iy)) ++nboth;
      se_merge_value<OFUSION>(ax, ay, sx, sy, mode, maxw, ix, iy);
      pa[lane + 64 * k] = ax;
      if (OFUSION) pa[512 + lane + 64 * k] = ay;
      else wb = (wb & ~(0xFFull << (8 * k))) | ((unsigned long long)(uint32_t)(int)ay << (8 * k));   // (an integer in 0 .. 255, as in k_merge_bricks)
    }
    if (!OFUSION) {
      wa.x = (uint32_t)wb; wa.y = (uint32_t)(wb >> 32);
      ((uint2*)(pa + 512))[lane] = wa;
    }
    if (lane == 0u) d.bactive[e - 1u] = 1;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) { nobs += __shfl_xor(nobs, o, 64); nboth += __shfl_xor(nboth, o, 64); }
  if (lane == 0u && nobs) { atomicAdd(&a.nvox[0], (unsigned long long)nobs); atomicAdd(&a.nvox[1], (unsigned long long)nboth); }
}
