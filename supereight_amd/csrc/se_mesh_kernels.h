// Map export, second half: marching cubes over the allocated blocks,
// se::algorithms::marching_cube (se_core/include/se/algorithms/meshing.hpp:161-208) as called by
// DenseSLAMSystem::dump_mesh (se_denseslam/src/DenseSLAMSystem.cpp:302-322): inside(v) = v.x < 0,
// select(v) = v.x.  One wave per block, lane = x + 8y, the 8 z-cells of a lane in turn; every cell reads
// its 8 corners through get_fine (a missing block reads initValue(), whose y == 0 ends the cell).
// Triangle table: include/se_mc_table.h (the standard published table, content-identical to the reference's edge_tables.h:66).
#pragma once
#include "../../include/se_mc_table.h"
#include "se_device.h"

__constant__ signed char SE_MC_TRI[256][SE_MC_WIDTH];

struct MeshArgs {
  float* out;                       // 9 floats per triangle, or null: count only
  unsigned long long* counter;      // [0] = triangles counted, [1] = triangles written
  unsigned long long capacity;      // triangles `out` can hold
};

// Octree::get_fine (octree.hpp:357-377)
__device__ __forceinline__ void se_get_fine(const DevMap& m, int x, int y, int z, float& vx, float& vy) {
  vx = m.init_x; vy = m.init_y;
  if (!in_volume(m, x, y, z)) return;
  uint32_t e = m.dense ? block_linear(m, x >> 3, y >> 3, z >> 3) + 1u : m.tab[leaf_index(m, x >> 3, y >> 3, z >> 3)];
  if (e == 0u || e == SE_PENDING) return;
  const size_t vi = (size_t)(e - 1u) * SE_BRICK_STRIDE + (size_t)((x & 7) + ((y & 7) << 3) + ((z & 7) << 6));
  vx = m.vx[vi]; vy = se_ld_y(m, vi);
}

// compute_intersection (meshing.hpp:45-55): s + (0.0 - v1) * (d - s) / (v2 - v1), coefficient-wise
__device__ __forceinline__ f3 se_mc_vertex(const DevMap& m, int x, int y, int z, int edge) {
  const int C[8][3] = {{0, 0, 0}, {1, 0, 0}, {1, 0, 1}, {0, 0, 1}, {0, 1, 0}, {1, 1, 0}, {1, 1, 1}, {0, 1, 1}};
  const int E[12][2] = {{0, 1}, {1, 2}, {2, 3}, {0, 3}, {4, 5}, {5, 6}, {6, 7}, {4, 7}, {0, 4}, {1, 5}, {2, 6}, {3, 7}};
  const int a = E[edge][0], b = E[edge][1];
  const int sx = x + C[a][0], sy = y + C[a][1], sz = z + C[a][2];
  const int dx = x + C[b][0], dy = y + C[b][1], dz = z + C[b][2];
  const float voxelSize = m.dim / m.size;
  const f3 s = {sx * voxelSize, sy * voxelSize, sz * voxelSize};
  const f3 d = {dx * voxelSize, dy * voxelSize, dz * voxelSize};
  float v1, v2, w;
  se_get_fine(m, sx, sy, sz, v1, w);
  se_get_fine(m, dx, dy, dz, v2, w);
  const float k = (float)(0.0 - (double)v1);
  return {s.x + (k * (d.x - s.x)) / (v2 - v1), s.y + (k * (d.y - s.y)) / (v2 - v1), s.z + (k * (d.z - s.z)) / (v2 - v1)};
}
__device__ __forceinline__ bool se_mc_reject(f3 v, float dim) { return v.x <= 0 || v.y <= 0 || v.z <= 0 || v.x > dim || v.y > dim || v.z > dim; }

__global__ __launch_bounds__(SE_WG) void k_mesh(DevMap m, MeshArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * SE_WG + threadIdx.x) >> 6;
  const int nwaves = (gridDim.x * SE_WG) >> 6;
  const uint32_t nblocks = min(m.ctr[C_BLOCKS], m.cap_blocks);
  const int C[8][3] = {{0, 0, 0}, {1, 0, 0}, {1, 0, 1}, {0, 0, 1}, {0, 1, 0}, {1, 1, 0}, {1, 1, 1}, {0, 1, 1}};
  for (uint32_t b = wave; b < nblocks; b += nwaves) {
    const uint32_t bp = m.bpos[b];
    const int bx = (int)(bp & 1023u) << 3, by = (int)((bp >> 10) & 1023u) << 3, bz = (int)(bp >> 20) << 3;
    const int x = bx + (lane & 7), y = by + (lane >> 3);
    // top = (coordinates + 8).cwiseMin(size - 1): cells whose +1 corner would leave the volume are skipped
    if (x >= min(bx + 8, m.size - 1) || y >= min(by + 8, m.size - 1)) continue;
    for (int z = bz; z < min(bz + 8, m.size - 1); ++z) {
      // compute_index (meshing.hpp:121-155)
      float px[8], py[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) se_get_fine(m, x + C[i][0], y + C[i][1], z + C[i][2], px[i], py[i]);
      bool known = true;
      unsigned index = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i) { known = known && !(py[i] == 0.f); index |= (px[i] < 0.f) ? (1u << i) : 0u; }
      if (!known) index = 0;
      const signed char* edges = SE_MC_TRI[index];
      for (unsigned e = 0; e < 16 && edges[e] != -1; e += 3) {
        const f3 v1 = se_mc_vertex(m, x, y, z, edges[e]);
        const f3 v2 = se_mc_vertex(m, x, y, z, edges[e + 1]);
        const f3 v3 = se_mc_vertex(m, x, y, z, edges[e + 2]);
        if (se_mc_reject(v1, m.dim) || se_mc_reject(v2, m.dim) || se_mc_reject(v3, m.dim)) continue;
        if (!a.out) { atomicAdd(&a.counter[0], 1ull); continue; }
        const unsigned long long slot = atomicAdd(&a.counter[1], 1ull);
        if (slot >= a.capacity) continue;
        float* o = a.out + 9 * slot;
        o[0] = v1.x; o[1] = v1.y; o[2] = v1.z; o[3] = v2.x; o[4] = v2.y; o[5] = v2.z; o[6] = v3.x; o[7] = v3.y; o[8] = v3.z;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Live meshing per block (se_hip_mesh_blocks, include/se_hip.h): the same cells, vertices and triangles as k_mesh, for the
// blocks a region and a set of views select, grouped per block, each block's triangles contiguous and in a defined order (cells x fastest,
// then y, then z; a cell's triangles in table order).
//
// One wave per block, lane = x + 8y.  The wave stages the 9 x 9 x 9 corner values its 8^3 cells read -- the block's own brick plus the +1
// layer of the up to 7 neighbour bricks in +x / +y / +z, each resolved once -- and a 'known' byte (y != 0) per corner in LDS: 729 floats
// + 729 bytes (SE_MB_TILE_BYTES = 3 680 per wave, 14 720 per workgroup).  Cells, vertices and rejections then come from LDS with
// se_mc_vertex's arithmetic, operation for operation.  Each lane counts its triangles per z slice, a wave prefix sum gives every triangle
// its place in the defined order, ONE atomic per block reserves the block's table slot and triangle range, and the lanes write.
#define SE_MB_TILE 729
#define SE_MB_TILE_PAD 736                       // floats per wave (known bytes follow)
#define SE_MB_TILE_BYTES (SE_MB_TILE_PAD * 5)    // 2 944 bytes of values + 736 known bytes = 3 680, a multiple of 16
#define SE_MB_MAX_VIEWS 64
#define SE_MB_VIEW_FLOATS 20                     // 5 planes (z > 0, left, right, top, bottom) x (nx, ny, nz, d), in voxel units
#define SE_MB_VIEWS_PER_LAUNCH 16
#define SE_MB_TRI_BITS 37                        // packed reservation counter: [blocks : 27][triangles : 37]
#define SE_MB_SKIP_EMPTY 1u

struct MeshBlocksArgs {
  int lo[3], hi[3];                 // region in voxels, clamped to the volume; never empty (the host does not launch then)
  int n_views;
  unsigned flags;
  const float* planes;              // [SE_MB_VIEW_FLOATS][SE_MB_MAX_VIEWS]: value j of view v at planes[j * 64 + v]
  unsigned long long* state;        // [0] packed reservation counter, [1] table slot and [2] first triangle of the first block that did not fit
  float* tri;                       // [cap_tri][9]
  int32_t* coords;                  // [cap_blk][3]
  long long* range;                 // [cap_blk][2]
  unsigned long long cap_tri, cap_blk;
};

struct MeshViewChunk { float v[SE_MB_VIEWS_PER_LAUNCH][SE_MB_VIEW_FLOATS]; };

// Resets the reservation state (base == 0) and copies up to 16 views' planes from the kernel arguments into the handle's buffer: the caller's
// selection has been read when the call returns, and nothing but stream order separates two calls.
__global__ void k_mesh_blocks_begin(MeshViewChunk c, int base, int n, float* planes, unsigned long long* state) {
  const int t = threadIdx.x;
  if (base == 0 && t == 0) { state[0] = 0ull; state[1] = ~0ull; state[2] = ~0ull; }
  for (int i = t; i < n * SE_MB_VIEW_FLOATS; i += blockDim.x) {
    const int v = i / SE_MB_VIEW_FLOATS, j = i - v * SE_MB_VIEW_FLOATS;
    planes[j * SE_MB_MAX_VIEWS + base + v] = c.v[v][j];
  }
}
// header: blocks selected, triangles needed, blocks written, triangles written.  Blocks are written in reservation order up to the first that
// does not fit (every later reservation starts behind it and fails too), so that block's slot and first triangle are the written totals.
__global__ void k_mesh_blocks_end(const unsigned long long* state, long long* header) {
  const unsigned long long blocks = state[0] >> SE_MB_TRI_BITS, tris = state[0] & ((1ull << SE_MB_TRI_BITS) - 1ull);
  header[0] = (long long)blocks; header[1] = (long long)tris;
  header[2] = (long long)(state[1] < blocks ? state[1] : blocks);
  header[3] = (long long)(state[2] < tris ? state[2] : tris);
}

// corner i of a cell -> (dx | dy << 1 | dz << 2), 3 bits each (C[8][3] of k_mesh); edge -> its two corners (E[12][2] of se_mc_vertex)
#define SE_MB_CORNERS 0x00DDA948u   /* 0, 1, 5, 4, 2, 3, 7, 6 */
#define SE_MB_EDGE_A 0x6889AC088ull /* 0, 1, 2, 0, 4, 5, 6, 4, 0, 1, 2, 3 */
#define SE_MB_EDGE_B 0xFACFF56D1ull /* 1, 2, 3, 3, 5, 6, 7, 7, 4, 5, 6, 7 */
__device__ __forceinline__ int se_mb_corner(int i) { return (int)((SE_MB_CORNERS >> (3 * i)) & 7u); }

// se_mc_vertex with the two corner values taken from the tile: (x, y, z) the cell, (lx, ly, lz) the same relative to the block
__device__ __forceinline__ f3 se_mb_vertex(const float* tile, float voxelSize, int x, int y, int z, int t, int edge) {
  const int ca = se_mb_corner((int)((SE_MB_EDGE_A >> (3 * edge)) & 7ull)), cb = se_mb_corner((int)((SE_MB_EDGE_B >> (3 * edge)) & 7ull));
  const int ax = ca & 1, ay = (ca >> 1) & 1, az = ca >> 2, bx = cb & 1, by = (cb >> 1) & 1, bz = cb >> 2;
  const int sx = x + ax, sy = y + ay, sz = z + az;
  const int dx = x + bx, dy = y + by, dz = z + bz;
  const f3 s = {sx * voxelSize, sy * voxelSize, sz * voxelSize};
  const f3 d = {dx * voxelSize, dy * voxelSize, dz * voxelSize};
  const float v1 = tile[t + ax + 9 * ay + 81 * az];
  const float v2 = tile[t + bx + 9 * by + 81 * bz];
  const float k = (float)(0.0 - (double)v1);
  return {s.x + (k * (d.x - s.x)) / (v2 - v1), s.y + (k * (d.y - s.y)) / (v2 - v1), s.z + (k * (d.z - s.z)) / (v2 - v1)};
}

// marching-cubes index of the cell at tile offset t (compute_index, as in k_mesh): 0 unless all 8 corners are known
__device__ __forceinline__ unsigned se_mb_index(const float* tile, const uint8_t* known, int t) {
  unsigned index = 0, kn = 1;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = se_mb_corner(i);
    const int o = t + (c & 1) + 9 * ((c >> 1) & 1) + 81 * (c >> 2);
    kn &= known[o];
    index |= (tile[o] < 0.f) ? (1u << i) : 0u;
  }
  return kn ? index : 0u;
}

template <bool DENSE>
__global__ __launch_bounds__(SE_WG) void k_mesh_blocks(DevMap m, MeshBlocksArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char s_all[(SE_WG / 64) * SE_MB_TILE_BYTES];
  const int lane = threadIdx.x & 63;
  float* tile = (float*)(s_all + (threadIdx.x >> 6) * SE_MB_TILE_BYTES);
  uint8_t* known = (uint8_t*)(tile + SE_MB_TILE_PAD);
  const int wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * SE_WG + threadIdx.x) >> 6));
  const int nwaves = (gridDim.x * SE_WG) >> 6;
  const uint32_t nblocks = min(m.ctr[C_BLOCKS], m.cap_blocks);
  const float voxelSize = m.dim / m.size;
  for (uint32_t b = wave; b < nblocks; b += nwaves) {
    const uint32_t bp = __builtin_amdgcn_readfirstlane(m.bpos[b]);
    const int bx = (int)(bp & 1023u) << 3, by = (int)((bp >> 10) & 1023u) << 3, bz = (int)(bp >> 20) << 3;
    // ---- selection: the region, then the views (lane v tests view v)
    if (bx >= a.hi[0] || bx + 8 <= a.lo[0] || by >= a.hi[1] || by + 8 <= a.lo[1] || bz >= a.hi[2] || bz + 8 <= a.lo[2]) continue;
    if (a.n_views > 0) {
      bool vis = false;
      if (lane < a.n_views) {
        const float cx = (float)(bx + 4), cy = (float)(by + 4), cz = (float)(bz + 4);   // centre of the 9^3 dependency box (exact in float)
        vis = true;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
          const float* q = a.planes + (4 * j) * SE_MB_MAX_VIEWS + lane;
          const float sd = ((q[0] * cx + q[SE_MB_MAX_VIEWS] * cy) + q[2 * SE_MB_MAX_VIEWS] * cz) + q[3 * SE_MB_MAX_VIEWS];
          vis = vis && sd > -9.f;
        }
      }
      if (__ballot(vis) == 0ull) continue;
    }
    // (the wave's previous block: every lane has finished reading the tile before any lane overwrites it.  A wave's LDS accesses complete in
    // order and the wave is the only user of its tile, so these are compiler fences, not hardware barriers)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // ---- stage the tile.  Own brick: slice z of the x plane is one coalesced row of 64 floats; the eight weights of an SDF column are one 8-byte word.
    const uint32_t slot = block_slot(m, b, bp);
    const float* brick = m.vx + (size_t)slot * SE_BRICK_STRIDE;
    const int t0 = (lane & 7) + 9 * (lane >> 3);
#pragma unroll
    for (int z = 0; z < 8; ++z) tile[t0 + 81 * z] = brick[lane + 64 * z];
    if (m.ybyte) {
      const uint2 w = *(const uint2*)((const uint8_t*)(brick + 512) + 8 * lane);   // bytes SE_YB(lane + 64 z) = 8 lane + z, z = 0 .. 7
#pragma unroll
      for (int z = 0; z < 8; ++z) known[t0 + 81 * z] = (((z < 4 ? w.x : w.y) >> (8 * (z & 3))) & 255u) != 0u;
    } else {
#pragma unroll
      for (int z = 0; z < 8; ++z) known[t0 + 81 * z] = !(brick[512 + lane + 64 * z] == 0.f);
    }
    // the 7 neighbours in +x / +y / +z: lane n (1 .. 7) resolves neighbour n = dx | dy << 1 | dz << 2 once; 0 = absent (reads initValue())
    uint32_t ne = 0u;
    {
      const int n = lane & 7;
      const int qx = (bx >> 3) + (n & 1), qy = (by >> 3) + ((n >> 1) & 1), qz = (bz >> 3) + (n >> 2);
      if (in_volume(m, qx << 3, qy << 3, qz << 3)) {
        ne = DENSE ? block_linear(m, qx, qy, qz) + 1u : m.tab[leaf_index(m, qx, qy, qz)];
        if (ne == SE_PENDING) ne = 0u;
      }
    }
    // the +1 layer: 217 corners with a coordinate equal to 8 -- three faces of 64, three edges of 8, one corner
    for (int i = lane; i < 217; i += 64) {
      int lx, ly, lz;
      if (i < 64) { lx = 8; ly = i & 7; lz = i >> 3; }
      else if (i < 128) { lx = i & 7; ly = 8; lz = (i >> 3) & 7; }
      else if (i < 192) { lx = i & 7; ly = (i >> 3) & 7; lz = 8; }
      else if (i < 200) { lx = 8; ly = 8; lz = i & 7; }
      else if (i < 208) { lx = 8; ly = i & 7; lz = 8; }
      else if (i < 216) { lx = i & 7; ly = 8; lz = 8; }
      else { lx = 8; ly = 8; lz = 8; }
      const int n = (lx >> 3) | ((ly >> 3) << 1) | ((lz >> 3) << 2);
      const uint32_t e = (uint32_t)__shfl((int)ne, n);
      float vx = m.init_x, vy = m.init_y;
      if (e != 0u) {
        const size_t vi = (size_t)(e - 1u) * SE_BRICK_STRIDE + (size_t)((lx & 7) + ((ly & 7) << 3) + ((lz & 7) << 6));
        vx = m.vx[vi]; vy = se_ld_y(m, vi);
      }
      const int o = lx + 9 * ly + 81 * lz;
      tile[o] = vx; known[o] = !(vy == 0.f);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // ---- pass 1: triangles per lane and z slice (4 bits each).  top = (coordinates + 8).cwiseMin(size - 1), as in k_mesh
    const int x = bx + (lane & 7), y = by + (lane >> 3);
    const bool live = x < min(bx + 8, m.size - 1) && y < min(by + 8, m.size - 1);
    const int nz = min(bz + 8, m.size - 1) - bz;
    uint32_t cnt = 0u;
    if (live) {
      for (int lz = 0; lz < nz; ++lz) {
        const int t = t0 + 81 * lz;
        const signed char* edges = SE_MC_TRI[se_mb_index(tile, known, t)];
        uint32_t c = 0u;
        for (unsigned e = 0; e < 16 && edges[e] != -1; e += 3) {
          const f3 v1 = se_mb_vertex(tile, voxelSize, x, y, bz + lz, t, edges[e]);
          const f3 v2 = se_mb_vertex(tile, voxelSize, x, y, bz + lz, t, edges[e + 1]);
          const f3 v3 = se_mb_vertex(tile, voxelSize, x, y, bz + lz, t, edges[e + 2]);
          if (se_mc_reject(v1, m.dim) || se_mc_reject(v2, m.dim) || se_mc_reject(v3, m.dim)) continue;
          ++c;
        }
        cnt |= c << (4 * lz);
      }
    }
    // ---- each lane's offset per z slice: slices in order, lanes in order within a slice
    uint32_t total = 0u;
    uint32_t off[8];
#pragma unroll
    for (int lz = 0; lz < 8; ++lz) {
      const uint32_t c = (cnt >> (4 * lz)) & 15u;
      uint32_t s = c;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) { const uint32_t u = (uint32_t)__shfl_up((int)s, d); if (lane >= d) s += u; }
      off[lz] = total + s - c;
      total += (uint32_t)__shfl((int)s, 63);
    }
    if (total == 0u && (a.flags & SE_MB_SKIP_EMPTY)) continue;
    // ---- one reservation per block: table slot and triangle range together
    unsigned long long r = 0ull;
    if (lane == 0) r = atomicAdd(&a.state[0], (1ull << SE_MB_TRI_BITS) | (unsigned long long)total);
    const unsigned long long islot = ((unsigned long long)(uint32_t)__shfl((int)(r >> 32), 0) << 32 | (uint32_t)__shfl((int)(uint32_t)r, 0));
    const unsigned long long tslot = islot >> SE_MB_TRI_BITS, first = islot & ((1ull << SE_MB_TRI_BITS) - 1ull);
    if (tslot >= a.cap_blk || first + total > a.cap_tri) {
      if (lane == 0) { atomicMin(&a.state[1], tslot); atomicMin(&a.state[2], first); }
      continue;
    }
    if (lane < 3) a.coords[3 * tslot + lane] = lane == 0 ? bx : (lane == 1 ? by : bz);
    if (lane < 2) a.range[2 * tslot + lane] = lane == 0 ? (long long)first : (long long)total;
    // ---- pass 2: the same cells again, written in place
    if (live) {
#pragma unroll
      for (int lz = 0; lz < 8; ++lz) {
        if (lz >= nz || ((cnt >> (4 * lz)) & 15u) == 0u) continue;
        const int t = t0 + 81 * lz;
        const signed char* edges = SE_MC_TRI[se_mb_index(tile, known, t)];
        float* o = a.tri + 9 * (first + off[lz]);
        for (unsigned e = 0; e < 16 && edges[e] != -1; e += 3) {
          const f3 v1 = se_mb_vertex(tile, voxelSize, x, y, bz + lz, t, edges[e]);
          const f3 v2 = se_mb_vertex(tile, voxelSize, x, y, bz + lz, t, edges[e + 1]);
          const f3 v3 = se_mb_vertex(tile, voxelSize, x, y, bz + lz, t, edges[e + 2]);
          if (se_mc_reject(v1, m.dim) || se_mc_reject(v2, m.dim) || se_mc_reject(v3, m.dim)) continue;
          o[0] = v1.x; o[1] = v1.y; o[2] = v1.z; o[3] = v2.x; o[4] = v2.y; o[5] = v2.z; o[6] = v3.x; o[7] = v3.y; o[8] = v3.z;
          o += 9;
        }
      }
    }
  }
}
