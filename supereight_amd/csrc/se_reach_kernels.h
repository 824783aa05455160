// The reachability field of a map region (se_hip_reach_field, include/se_hip.h): a wavefront / NF1 navigation function over the C-space of the
// box robot that se_hip_distance_field models.  Position v of the region [lo, lo + side) is free iff no voxel of [v, v + robot) blocks; moves
// are 6-connected between free positions of the region; key(v) = steps(v) * 256 + seed(v) is the unique solution of
//     key(v) = min(own seed index if any, min over free neighbours u of key(u) + 256).
// The host restatement, the literal definition and the proof of the round bound are include/se/reach_field.hpp and DESIGN.md 4.22.
//
// Launches, all plain, on the handle's stream; termination belongs to the host (se_hip_api.hip), every launch always ends:
//   k_field_classify  (se_field_kernels.h, unchanged) over the block-aligned hull of the C-space domain [lo, lo + side + robot - 1): blocking
//                     bits in rows along x.  It writes bytes 0 .. nb[0] - 1 of a row only; nothing below reads a bit beyond 8 nb[0].
//   k_reach_free<P>   three separable passes over 64-bit words, one lane per output word, each an OR over a window of `robot` <= 256:
//                     P = 0  wx[z'][y'][w] = OR over s < robot_x of the 64 blocking bits from x = lo_x + 64 w + s on      (D_z x D_y rows)
//                     P = 1  wy[z'][j][w]  = OR over t < robot_y of wx[z'][j + t][w]                                      (D_z x side_y rows)
//                     P = 2  free[k][j][w] = NOT OR over t < robot_z of wy[k + t][j][w], bits beyond side_x cleared       (side_z x side_y rows)
//                     with D = side + robot - 1.  For robot (1, 1, 1) every window is one item: a complement.
//   k_reach_seed      one lane per seed: a seed inside the region whose free bit is set writes atomicMin(key, index) (the key array was filled
//                     with SE_REACH_NOKEY before), marks its tile dirty for round 1 and, where it lies on a face of its tile, the tile across
//                     that face too.  The seed coordinates are compared in 64 bits: any int32 is a valid, if unusable, seed.
//   k_reach_relax     the hot path, one workgroup of 256 lanes per 32 x 8 x 8 tile (128-byte rows of keys), launched once per round.  A tile
//                     whose mark of this round's parity is clear exits at once; else the mark is cleared, the tile's keys and a one-cell halo
//                     (34 x 10 x 10 x 4 B = 13 600 B of LDS) are loaded -- outside the region: no key -- and the tile is relaxed to its local
//                     fixed point in gather form, key = min(key, min over the six neighbours + 256) under the free bit.  Lane (x, y) owns the
//                     column z = 0 .. 7 of its tile: it reads LDS, a barrier, it writes its own cells, and __syncthreads_or decides the exit
//                     for the whole workgroup; at most SE_REACH_TILE_CELLS + 1 iterations (a key that changes decreases, and a cell's key
//                     takes at most one value per length of a path inside the tile).  Then every own cell that decreased is written back, and
//                     for every face on which a cell decreased the tile across it is marked in the OTHER parity and `changed` is bumped.
//                     Halo keys that another workgroup rewrites during the same launch may be read stale: every value ever stored is an upper
//                     bound of the final key, keys only decrease, and the writer marks this tile for the next round.
//   k_reach_finish    one lane per position: steps / seed from the key, next from the six neighbour keys (the lowest direction whose
//                     neighbour holds key - 256), the three counts by a wave reduction and one atomic per count and workgroup.
// Every index is formed in size_t from quantities the host has checked (positions <= 2^24, robot <= 256, |coordinates| <= 2^19).  Reads of
// the bit rows stay inside [0, words); reads and writes of keys inside the region.
#pragma once
#include "se_field_kernels.h"

#define SE_REACH_NOKEY 0xFFFFFFFFu
#define SE_REACH_NONE (-1)
#define SE_REACH_AT_SEED 6
#define SE_REACH_MAX_SEEDS 255
#define SE_REACH_TX 32
#define SE_REACH_TY 8
#define SE_REACH_TZ 8
#define SE_REACH_TILE_CELLS (SE_REACH_TX * SE_REACH_TY * SE_REACH_TZ)
#define SE_WG_REACH 256

struct ReachArgs {
  int lo[3], side[3], robot[3];
  int D[3];                        // the C-space domain's cells per axis: side + robot - 1
  HullArgs hull;                   // the hull of k_field_classify: blocking bits [8 nb[2]][8 nb[1]][words]
  int wr;                          // 64-bit words per row of the region: ceil(side[0] / 64)
  int nt[3];                       // tiles per axis
  int n_seeds;
  unsigned long long* wx;          // [D[2]][D[1]][wr]
  unsigned long long* wy;          // [D[2]][side[1]][wr]
  unsigned long long* free;        // [side[2]][side[1]][wr]
  unsigned long long* counts;      // [0] free, [1] reached, [2] max steps + 1
  uint32_t* key;                   // [side[2]][side[1]][side[0]]
  uint32_t* dirty;                 // [2][tiles]: marks by round parity
  uint32_t* changed;               // marks made since the call began
  const int32_t* seeds;            // [n_seeds][3]
  int32_t* steps; uint8_t* seed; uint8_t* next;
};

// 64 bits of a row from bit `from` (>= 0) on; words beyond the row read as zero
__device__ __forceinline__ unsigned long long se_reach_extract(const unsigned long long* row, int words, int from) {
  const int w = from >> 6, s = from & 63;
  const unsigned long long a = w < words ? row[w] : 0ull, b = (s && w + 1 < words) ? row[w + 1] : 0ull;
  return s ? (a >> s) | (b << (64 - s)) : a;
}

template <int PASS>
__global__ __launch_bounds__(SE_WG_REACH) void k_reach_free(ReachArgs a) {
  const size_t wr = (size_t)a.wr;
  const size_t rows_y = PASS == 0 ? (size_t)a.D[1] : (size_t)a.side[1], rows_z = PASS == 2 ? (size_t)a.side[2] : (size_t)a.D[2];
  const size_t total = wr * rows_y * rows_z;
  const int window = min(a.robot[PASS], SE_FIELD_ROBOT);
  for (size_t idx = (size_t)blockIdx.x * SE_WG_REACH + threadIdx.x; idx < total; idx += (size_t)gridDim.x * SE_WG_REACH) {
    const size_t w = idx % wr, y = (idx / wr) % rows_y, z = idx / (wr * rows_y);
    unsigned long long acc = 0ull;
    if (PASS == 0) {
      // the domain's origin inside the hull, per axis: lo - 8 b0, in [0, 8)
      const int hx = a.lo[0] - 8 * a.hull.b0[0], hy = a.lo[1] - 8 * a.hull.b0[1], hz = a.lo[2] - 8 * a.hull.b0[2];
      const unsigned long long* row = a.hull.bits + ((z + (size_t)hz) * ((size_t)a.hull.nb[1] * 8u) + (y + (size_t)hy)) * (size_t)a.hull.words;
      for (int s = 0; s < window; ++s) acc |= se_reach_extract(row, a.hull.words, hx + 64 * (int)w + s);
      a.wx[idx] = acc;
    } else if (PASS == 1) {
      const unsigned long long* col = a.wx + (z * (size_t)a.D[1] + y) * wr + w;
      for (int t = 0; t < window; ++t) acc |= col[(size_t)t * wr];
      a.wy[idx] = acc;
    } else {
      const size_t plane = (size_t)a.side[1] * wr;
      const unsigned long long* col = a.wy + z * plane + y * wr + w;
      for (int t = 0; t < window; ++t) acc |= col[(size_t)t * plane];
      const int left = a.side[0] - 64 * (int)w;   // positions of the row from this word on: >= 1
      a.free[idx] = ~acc & (left >= 64 ? ~0ull : ~(~0ull << left));
    }
  }
}

__device__ __forceinline__ size_t se_reach_tile(const ReachArgs& a, int tx, int ty, int tz) {
  return ((size_t)tz * (size_t)a.nt[1] + (size_t)ty) * (size_t)a.nt[0] + (size_t)tx;
}

// (launched with one workgroup: n_seeds <= 255 < SE_WG_REACH)
__global__ __launch_bounds__(SE_WG_REACH) void k_reach_seed(ReachArgs a) {
  const int i = (int)threadIdx.x;
  if (blockIdx.x != 0u || i >= a.n_seeds) return;
  const long long x = (long long)a.seeds[3 * i] - a.lo[0], y = (long long)a.seeds[3 * i + 1] - a.lo[1], z = (long long)a.seeds[3 * i + 2] - a.lo[2];
  if (x < 0 || y < 0 || z < 0 || x >= a.side[0] || y >= a.side[1] || z >= a.side[2]) return;
  const size_t row = (size_t)z * (size_t)a.side[1] + (size_t)y;
  if (!((a.free[row * (size_t)a.wr + (size_t)(x >> 6)] >> (x & 63)) & 1ull)) return;
  atomicMin(a.key + row * (size_t)a.side[0] + (size_t)x, (uint32_t)i);
  // round 1 reads the marks of parity 1
  const size_t tiles = (size_t)a.nt[0] * (size_t)a.nt[1] * (size_t)a.nt[2];
  uint32_t* mark = a.dirty + tiles;
  const int tx = (int)x / SE_REACH_TX, ty = (int)y / SE_REACH_TY, tz = (int)z / SE_REACH_TZ;
  const int lx = (int)x % SE_REACH_TX, ly = (int)y % SE_REACH_TY, lz = (int)z % SE_REACH_TZ;
  mark[se_reach_tile(a, tx, ty, tz)] = 1u;
  if (lx == 0 && tx > 0) mark[se_reach_tile(a, tx - 1, ty, tz)] = 1u;
  if (lx == SE_REACH_TX - 1 && tx + 1 < a.nt[0]) mark[se_reach_tile(a, tx + 1, ty, tz)] = 1u;
  if (ly == 0 && ty > 0) mark[se_reach_tile(a, tx, ty - 1, tz)] = 1u;
  if (ly == SE_REACH_TY - 1 && ty + 1 < a.nt[1]) mark[se_reach_tile(a, tx, ty + 1, tz)] = 1u;
  if (lz == 0 && tz > 0) mark[se_reach_tile(a, tx, ty, tz - 1)] = 1u;
  if (lz == SE_REACH_TZ - 1 && tz + 1 < a.nt[2]) mark[se_reach_tile(a, tx, ty, tz + 1)] = 1u;
}

// a neighbour's key plus one move; no key stays no key (a real key is at most (2^24 - 1) * 256 + 254, and its seed byte is never 255)
__device__ __forceinline__ uint32_t se_reach_step(uint32_t k) { return k < 0xFFFFFF00u ? k + 256u : SE_REACH_NOKEY; }

#define SE_REACH_HX (SE_REACH_TX + 2)
#define SE_REACH_HY (SE_REACH_TY + 2)
#define SE_REACH_HZ (SE_REACH_TZ + 2)

__global__ __launch_bounds__(SE_WG_REACH) void k_reach_relax(ReachArgs a, uint32_t round) {
  __shared__ uint32_t tile[SE_REACH_HZ][SE_REACH_HY][SE_REACH_HX];
  __shared__ uint32_t faces;
  const size_t tiles = (size_t)a.nt[0] * (size_t)a.nt[1] * (size_t)a.nt[2];
  const size_t t = blockIdx.x;   // (the grid is the tile count)
  uint32_t* cur = a.dirty + (size_t)(round & 1u) * tiles;
  uint32_t* nxt = a.dirty + (size_t)((round & 1u) ^ 1u) * tiles;
  if (cur[t] == 0u) return;      // (uniform: one word for the whole workgroup)
  const int tx = (int)(t % (size_t)a.nt[0]), ty = (int)((t / (size_t)a.nt[0]) % (size_t)a.nt[1]), tz = (int)(t / ((size_t)a.nt[0] * (size_t)a.nt[1]));
  const int ox = tx * SE_REACH_TX, oy = ty * SE_REACH_TY, oz = tz * SE_REACH_TZ;   // the tile's origin in the region
  const int sx = a.side[0], sy = a.side[1], sz = a.side[2];
  const uint32_t tid = threadIdx.x;
  if (tid == 0u) faces = 0u;
  // the tile and its halo; outside the region there is no key
  for (uint32_t c = tid; c < (uint32_t)(SE_REACH_HX * SE_REACH_HY * SE_REACH_HZ); c += SE_WG_REACH) {
    const int hx = (int)(c % SE_REACH_HX), hy = (int)((c / SE_REACH_HX) % SE_REACH_HY), hz = (int)(c / (SE_REACH_HX * SE_REACH_HY));
    const int x = ox + hx - 1, y = oy + hy - 1, z = oz + hz - 1;
    uint32_t k = SE_REACH_NOKEY;
    if ((unsigned)x < (unsigned)sx && (unsigned)y < (unsigned)sy && (unsigned)z < (unsigned)sz) k = a.key[((size_t)z * (size_t)sy + (size_t)y) * (size_t)sx + (size_t)x];
    tile[hz][hy][hx] = k;
  }
  // the lane's column: (lx, ly), z = 0 .. 7; its free bits and the keys it found
  const int lx = (int)(tid & 31u), ly = (int)(tid >> 5);
  const int x = ox + lx, y = oy + ly;
  uint32_t freem = 0u;
  if (x < sx && y < sy) {
#pragma unroll
    for (int k = 0; k < SE_REACH_TZ; ++k)
      if (oz + k < sz) freem |= (uint32_t)((a.free[((size_t)(oz + k) * (size_t)sy + (size_t)y) * (size_t)a.wr + (size_t)(x >> 6)] >> (x & 63)) & 1ull) << k;
  }
  __syncthreads();
  if (tid == 0u) cur[t] = 0u;    // consumed (behind the barrier: every lane has read it)
  uint32_t k0[SE_REACH_TZ], kc[SE_REACH_TZ];
#pragma unroll
  for (int k = 0; k < SE_REACH_TZ; ++k) k0[k] = kc[k] = tile[k + 1][ly + 1][lx + 1];
  for (int it = 0; it <= SE_REACH_TILE_CELLS; ++it) {
    uint32_t any = 0u;
#pragma unroll
    for (int k = 0; k < SE_REACH_TZ; ++k) {
      const uint32_t n = min(min(min(tile[k + 1][ly + 1][lx], tile[k + 1][ly + 1][lx + 2]), min(tile[k + 1][ly][lx + 1], tile[k + 1][ly + 2][lx + 1])),
                             min(tile[k][ly + 1][lx + 1], tile[k + 2][ly + 1][lx + 1]));
      const uint32_t v = ((freem >> k) & 1u) ? min(kc[k], se_reach_step(n)) : kc[k];
      any |= (uint32_t)(v != kc[k]);
      kc[k] = v;
    }
    __syncthreads();             // every lane has read the old keys
    if (any) {
#pragma unroll
      for (int k = 0; k < SE_REACH_TZ; ++k) tile[k + 1][ly + 1][lx + 1] = kc[k];
    }
    if (!__syncthreads_or((int)any)) break;   // (a barrier, and the same answer in every lane)
  }
  // write back what decreased; the faces on which it did
  uint32_t f = 0u;
  if (x < sx && y < sy) {
#pragma unroll
    for (int k = 0; k < SE_REACH_TZ; ++k) {
      if (kc[k] != k0[k]) {
        a.key[((size_t)(oz + k) * (size_t)sy + (size_t)y) * (size_t)sx + (size_t)x] = kc[k];
        f |= (lx == 0 ? 1u : 0u) | (lx == SE_REACH_TX - 1 ? 2u : 0u) | (ly == 0 ? 4u : 0u) | (ly == SE_REACH_TY - 1 ? 8u : 0u) |
             (k == 0 ? 16u : 0u) | (k == SE_REACH_TZ - 1 ? 32u : 0u);
      }
    }
  }
  if (f) atomicOr(&faces, f);    // (LDS)
  __syncthreads();
  if (tid == 0u) {
    const uint32_t m = faces;
    uint32_t marks = 0u;
    if ((m & 1u) && tx > 0) { nxt[se_reach_tile(a, tx - 1, ty, tz)] = 1u; ++marks; }
    if ((m & 2u) && tx + 1 < a.nt[0]) { nxt[se_reach_tile(a, tx + 1, ty, tz)] = 1u; ++marks; }
    if ((m & 4u) && ty > 0) { nxt[se_reach_tile(a, tx, ty - 1, tz)] = 1u; ++marks; }
    if ((m & 8u) && ty + 1 < a.nt[1]) { nxt[se_reach_tile(a, tx, ty + 1, tz)] = 1u; ++marks; }
    if ((m & 16u) && tz > 0) { nxt[se_reach_tile(a, tx, ty, tz - 1)] = 1u; ++marks; }
    if ((m & 32u) && tz + 1 < a.nt[2]) { nxt[se_reach_tile(a, tx, ty, tz + 1)] = 1u; ++marks; }
    if (marks) atomicAdd(a.changed, marks);
  }
}

__global__ __launch_bounds__(SE_WG_REACH) void k_reach_finish(ReachArgs a) {
  const size_t s0 = (size_t)a.side[0], s1 = (size_t)a.side[1], s2 = (size_t)a.side[2], plane = s0 * s1, total = plane * s2;
  unsigned long long n_free = 0ull, n_reached = 0ull, top = 0ull;   // (top: max steps + 1)
  for (size_t idx = (size_t)blockIdx.x * SE_WG_REACH + threadIdx.x; idx < total; idx += (size_t)gridDim.x * SE_WG_REACH) {
    const size_t i = idx % s0, j = (idx / s0) % s1, k = idx / plane;
    const uint32_t key = a.key[idx];
    n_free += (a.free[(k * s1 + j) * (size_t)a.wr + (i >> 6)] >> (i & 63)) & 1ull;
    int32_t steps = SE_REACH_NONE;
    uint32_t seed = 255u, next = 255u;
    if (key != SE_REACH_NOKEY) {
      steps = (int32_t)(key >> 8);
      seed = key & 255u;
      ++n_reached;
      top = max(top, (unsigned long long)steps + 1ull);
      next = SE_REACH_AT_SEED;
      if (steps > 0) {
        const uint32_t want = key - 256u;
        // (descending, so that the lowest qualifying direction is the one kept)
        if (k + 1 < s2 && a.key[idx + plane] == want) next = 5u;
        if (k > 0 && a.key[idx - plane] == want) next = 4u;
        if (j + 1 < s1 && a.key[idx + s0] == want) next = 3u;
        if (j > 0 && a.key[idx - s0] == want) next = 2u;
        if (i + 1 < s0 && a.key[idx + 1] == want) next = 1u;
        if (i > 0 && a.key[idx - 1] == want) next = 0u;
      }
    }
    a.steps[idx] = steps;
    if (a.seed) a.seed[idx] = (uint8_t)seed;
    if (a.next) a.next[idx] = (uint8_t)next;
  }
  // a wave reduction, then one atomic per count and workgroup
  __shared__ unsigned long long part[3][SE_WG_REACH / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    n_free += __shfl_down(n_free, off, 64);
    n_reached += __shfl_down(n_reached, off, 64);
    top = max(top, (unsigned long long)__shfl_down(top, off, 64));
  }
  if ((threadIdx.x & 63u) == 0u) { part[0][threadIdx.x >> 6] = n_free; part[1][threadIdx.x >> 6] = n_reached; part[2][threadIdx.x >> 6] = top; }
  __syncthreads();
  if (threadIdx.x == 0u) {
    unsigned long long f = 0ull, r = 0ull, m = 0ull;
#pragma unroll
    for (int w = 0; w < SE_WG_REACH / 64; ++w) { f += part[0][w]; r += part[1][w]; m = max(m, part[2][w]); }
    if (f) atomicAdd(a.counts + 0, f);
    if (r) atomicAdd(a.counts + 1, r);
    if (m) atomicMax(a.counts + 2, m);
  }
}
