// Reading the field at a point: what the raycast, the volume renderer, the batched ray cast and the batched point query inline -- get(), Octree::interp
// (se_core/include/se/octree.hpp:541-563, gather_points: interp_gather.hpp:107-237) and Octree::grad (octree.hpp:652-737) on the brick layouts of
// se_device.h.  This header owns the addressing and the two blends and knows nothing about rays.
//
//   SeDense<O32>            dense grid: a voxel's index as a sum of one term per axis; O32 = 32-bit byte offsets (maps <= 4 GiB), else (block, local) pairs
//   se_sample_lean          one get() on the dense grid            SeSample<O32>
//   se_sample_pooled        one get() behind the leaf index        SePSample, SePCache (the previous sample's block and its entry)
//   se_cell_lean            the interpolation cell on the dense grid: fractions and eight corner indices (SeCell<O32>)
//   se_interp_generic       interp, every corner looked up in the block that holds it (2x2x2 candidate blocks)
//   se_interp_lean<O32>     interp on the dense grid from per-axis terms
//   se_grad_generic         grad, the 32 voxels picked from the 2x2x2 blocks of the stencil's extreme coordinates
//   se_grad_lean<O32>       grad on the dense grid from per-axis terms
//   se_grad_checked         grad, every voxel looked up by itself
//   se_hit_grad             the normal at a hit: the form that is exact where the hit lies
//   se_trilerp, se_grad_blend, se_stencil / se_stencil4, SE_GRAD_BAND      the two blends in the reference's term order, the stencil clamp, the band test: each once
//
// A missing block.  interp: a corner in a block that is not allocated, or outside the volume, reads empty().x -- initValue().x in the all-cross case
// (the cell straddles a block face on all three axes: gather_points goes through get_fine there).  grad: such a voxel reads initValue().x (the cached
// Octree::get(x, y, z, block) falls back to the tree walk, octree.hpp:379-408).  The values are identical for both field types.  On the dense grid every
// brick exists and is pre-filled with initValue(), so the lean forms read it without asking the index.
// Where each form is exact, and what it falls back to:
//   se_interp_generic   everywhere (a corner outside the volume has no block entry).
//   se_interp_lean      dense grid, the whole cell inside the volume (max(floor(q), 0) < size - 1 on every axis); else se_interp_generic<true>.
//   se_grad_generic     -1 <= floor(q) <= size - 1 on every axis (SE_GRAD_BAND): the stencil's voxels then lie in the blocks of its two extreme clamped
//                       coordinates per axis.  Outside that band the reference's `lower` index, clamped from below only, leaves the volume: se_grad_checked.
//   se_grad_lean        dense grid, floor(q) <= size - 1 on every axis; else se_grad_generic<true> (callers stay inside the band: se_hit_grad, k_query_points).
//   se_grad_checked     everywhere; 32 dependent look-ups, so only outside the band.
// The lean forms convert float -> int with the hardware instruction (se_cvt_hw), the generic and checked ones as cvttss2si does (cvt_i32); they agree
// for non-NaN |f| < 2^31 (se_device.h).
// Why unconditional loads.  Memory-level parallelism is what the raycast kernel lives on: a wave is a chain of dependent L2 round trips, so interp and
// grad are written as "all block look-ups -> all voxel loads -> math", a missing block reading a dummy address (voxel 0 of brick 0) whose value is
// replaced afterwards, instead of one branch per sample.
#pragma once
#include "se_device.h"

struct BlkCache { int bx, by, bz; uint32_t e; };
// voxel_traits<T>::initValue() / empty() as register values.  Reading them through the by-value
// DevMap inside `cond ? load : m.init_x` lets the compiler fold both into one FLAT load of a
// selected address (and park the constants in scratch to have an address).
struct FieldConst { float init_x, init_y, empty_x; };
__device__ __forceinline__ FieldConst se_field_const(const DevMap& m) {
  FieldConst f = {m.init_x, m.init_y, m.empty_x};
  asm volatile("" : "+s"(f.init_x), "+s"(f.init_y), "+s"(f.empty_x));
  return f;
}

__device__ __forceinline__ size_t se_voxel_index(uint32_t e, int x, int y, int z) {
  return (size_t)(e - 1u) * SE_BRICK_STRIDE + (size_t)((x & 7) + ((y & 7) << 3) + ((z & 7) << 6));
}

// Octree::interp's blend of the eight corners p[i + 2j + 4k] (octree.hpp:553-562), same term order
__device__ __forceinline__ float se_trilerp(const float (&p)[8], float fx, float fy, float fz) {
  return (((p[0] * (1 - fx) + p[1] * fx) * (1 - fy) + (p[2] * (1 - fx) + p[3] * fx) * fy) * (1 - fz) +
          ((p[4] * (1 - fx) + p[5] * fx) * (1 - fy) + (p[6] * (1 - fx) + p[7] * fx) * fy) * fz);
}
// Octree::grad's blend (octree.hpp:652-737), same term order.  V[zi][yi][xi] over the four clamped coordinates of each axis (se_stencil4: "lower" = 1,
// "upper" = 2); only the 32 entries with at least two axes on a central index are read.  The caller applies (0.5f * dim / size).
__device__ __forceinline__ f3 se_grad_blend(const float (&V)[4][4][4], float fx, float fy, float fz) {
  f3 g;
  g.x = (((V[1][1][2] - V[1][1][0]) * (1 - fx) + (V[1][1][3] - V[1][1][1]) * fx) * (1 - fy) +
         ((V[1][2][2] - V[1][2][0]) * (1 - fx) + (V[1][2][3] - V[1][2][1]) * fx) * fy) * (1 - fz) +
        (((V[2][1][2] - V[2][1][0]) * (1 - fx) + (V[2][1][3] - V[2][1][1]) * fx) * (1 - fy) +
         ((V[2][2][2] - V[2][2][0]) * (1 - fx) + (V[2][2][3] - V[2][2][1]) * fx) * fy) * fz;
  g.y = (((V[1][2][1] - V[1][0][1]) * (1 - fx) + (V[1][2][2] - V[1][0][2]) * fx) * (1 - fy) +
         ((V[1][3][1] - V[1][1][1]) * (1 - fx) + (V[1][3][2] - V[1][1][2]) * fx) * fy) * (1 - fz) +
        (((V[2][2][1] - V[2][0][1]) * (1 - fx) + (V[2][2][2] - V[2][0][2]) * fx) * (1 - fy) +
         ((V[2][3][1] - V[2][1][1]) * (1 - fx) + (V[2][3][2] - V[2][1][2]) * fx) * fy) * fz;
  g.z = (((V[2][1][1] - V[0][1][1]) * (1 - fx) + (V[2][1][2] - V[0][1][2]) * fx) * (1 - fy) +
         ((V[2][2][1] - V[0][2][1]) * (1 - fx) + (V[2][2][2] - V[0][2][2]) * fx) * fy) * (1 - fz) +
        (((V[3][1][1] - V[1][1][1]) * (1 - fx) + (V[3][1][2] - V[1][1][2]) * fx) * (1 - fy) +
         ((V[3][2][1] - V[1][2][1]) * (1 - fx) + (V[3][2][2] - V[1][2][2]) * fx) * fy) * fz;
  return g;
}
// the four clamped stencil coordinates of an axis, {base - 1, base, base + 1, base + 2}[i] for base = floor(q): the lower two are clamped from below
// only, the upper two from above only (octree.hpp:658-669).  `i` is a constant at every call.  se_stencil4 gives all four to the forms that keep the
// coordinates (block and offset of each); se_grad_lean turns each into its axis term at once and takes them one by one.
// (Two forms of one rule on purpose: with se_stencil4 written on top of se_stencil, or either form used for all three gradients, the compiled
// kernels change.  profiles/march_fold_asm.txt lists what was tried; recheck the assembly before merging them.)
__device__ __forceinline__ int se_stencil(int b, int hi, int i) { return i < 2 ? max(b + i - 1, 0) : min(b + i - 1, hi); }
__device__ __forceinline__ void se_stencil4(int b, int hi, int (&c)[4]) {
  c[0] = max(b - 1, 0); c[1] = max(b, 0); c[2] = min(b + 1, hi); c[3] = min(b + 2, hi);
}
// The band of se_grad_generic / se_grad_lean (header comment): -1 <= b <= hi = size - 1 on every axis, for b = cvt_i32(floorf(q)).  Outside it
// se_grad_checked.  (A macro on purpose: as an inline function, in any of three shapes, the test changes the compiled raycast and query kernels.
// profiles/march_fold_asm.txt; recheck the assembly before turning it into a function.)
#define SE_GRAD_BAND(bx, by, bz, hi) ((bx) >= -1 && (bx) <= (hi) && (by) >= -1 && (by) <= (hi) && (bz) >= -1 && (bz) <= (hi))

// leaf-grid entry of block (bx,by,bz) or 0 outside the volume; `hint` is a block whose entry is
// already known (the block of the preceding get) and saves the load.
template <bool DENSE>
__device__ __forceinline__ uint32_t se_block_entry(const DevMap& m, int bx, int by, int bz, const BlkCache& hint) {
  const int nb = m.size >> 3;
  uint32_t e = 0u;
  if (DENSE) return ((unsigned)bx < (unsigned)nb && (unsigned)by < (unsigned)nb && (unsigned)bz < (unsigned)nb) ? block_linear(m, bx, by, bz) + 1u : 0u;
  if (bx == hint.bx && by == hint.by && bz == hint.bz) e = hint.e;
  else if ((unsigned)bx < (unsigned)nb && (unsigned)by < (unsigned)nb && (unsigned)bz < (unsigned)nb) e = m.tab[leaf_index(m, bx, by, bz)];
  // Pooled bricks: the allocation scan of the NEXT frame may be inserting blocks while this raycast runs (overlap mode).  An
  // entry in flight reads as PENDING -> "not allocated"; one already published points at a brick that still holds
  // initValue() in every voxel (bricks are pre-filled and never recycled), which is exactly what "not allocated" reads as
  // (initValue().x == empty().x for both field types) -- so the race cannot change a result.
  return e == SE_PENDING ? 0u : e;
}
// leaf-grid entry (slot + 1) of block (bx, by, bz), 0 if it lies outside the volume or is not allocated.  Both layouts keep
// the entry in tab[] (a dense brick grid also holds bricks of blocks that were never allocated: initValue() everywhere).
__device__ __forceinline__ uint32_t se_query_block(const DevMap& m, int bx, int by, int bz) {
  const int nb = m.size >> 3;
  if (!((unsigned)bx < (unsigned)nb && (unsigned)by < (unsigned)nb && (unsigned)bz < (unsigned)nb)) return 0u;
  const uint32_t e = m.tab[leaf_index(m, bx, by, bz)];
  return e == SE_PENDING ? 0u : e;
}

// Octree::interp with gather_points: every corner is read from the block that contains it.
template <bool DENSE>
__device__ __forceinline__ float se_interp_generic(const DevMap& m, const FieldConst fc, f3 pos, BlkCache& c) {
  const float flx = floorf(pos.x), fly = floorf(pos.y), flz = floorf(pos.z);
  const int bx = cvt_i32(flx), by = cvt_i32(fly), bz = cvt_i32(flz);
  const float fx = pos.x - flx, fy = pos.y - fly, fz = pos.z - flz;
  const int lx = max(bx, 0), ly = max(by, 0), lz = max(bz, 0);
  const bool cx = (lx & 7) == 7, cy = (ly & 7) == 7, cz = (lz & 7) == 7;
  const float missing = (cx && cy && cz) ? fc.init_x : fc.empty_x;
  // phase 1: the (up to 8) blocks the cell touches
  uint32_t e[8];
  e[0] = se_block_entry<DENSE>(m, lx >> 3, ly >> 3, lz >> 3, c);
#pragma unroll
  for (int k = 1; k < 8; ++k) {
    const bool need = (!(k & 1) || cx) && (!(k & 2) || cy) && (!(k & 4) || cz);
    e[k] = 0u;
    if (need) e[k] = se_block_entry<DENSE>(m, (lx + (k & 1)) >> 3, (ly + ((k >> 1) & 1)) >> 3, (lz + (k >> 2)) >> 3, c);
  }
  // phase 2: the 8 corner values.  Corner (i, j, k) lies in block (i && cx, j && cy, k && cz) of the 2x2x2 candidates: the entry is picked axis by
  // axis (12 selects for the cell; r04 -- a chain of seven compares and selects per corner before) and the voxel offset is a sum of per-axis terms
  uint32_t ex1[4], exy[2][2][2];     // ex1[q] = the x-upper corner's entry for (y, z) block pair q; exy[i][j][s] after the y step
#pragma unroll
  for (int q = 0; q < 4; ++q) ex1[q] = cx ? e[2 * q + 1] : e[2 * q];
#pragma unroll
  for (int sz = 0; sz < 2; ++sz) {
    exy[0][0][sz] = e[4 * sz];
    exy[1][0][sz] = ex1[2 * sz];
    exy[0][1][sz] = cy ? e[4 * sz + 2] : e[4 * sz];
    exy[1][1][sz] = cy ? ex1[2 * sz + 1] : ex1[2 * sz];
  }
  const uint32_t ox[2] = {(uint32_t)lx & 7u, (uint32_t)(lx + 1) & 7u};
  const uint32_t oy[2] = {((uint32_t)ly & 7u) << 3, ((uint32_t)(ly + 1) & 7u) << 3};
  const uint32_t oz[2] = {((uint32_t)lz & 7u) << 6, ((uint32_t)(lz + 1) & 7u) << 6};
  float p[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int i = k & 1, j = (k >> 1) & 1, kz = k >> 2;
    const uint32_t ek = kz ? (cz ? exy[i][j][1] : exy[i][j][0]) : exy[i][j][0];
    const size_t vi = ek ? (size_t)(ek - 1u) * SE_BRICK_STRIDE + (size_t)(ox[i] + oy[j] + oz[kz]) : 0;
    const float v = m.vx[vi];
    p[k] = ek ? v : missing;
  }
  return se_trilerp(p, fx, fy, fz);
}

// Octree::grad.  The 48 get() calls of the reference touch 32 distinct voxels: per axis the four clamped coordinates of se_stencil4, every sample
// having at least two axes on a central index.  They lie in at most 2x2x2 blocks.
template <bool DENSE>
__device__ __forceinline__ f3 se_grad_generic(const DevMap& m, const FieldConst fc, f3 pos, BlkCache& c) {
  const float flx = floorf(pos.x), fly = floorf(pos.y), flz = floorf(pos.z);
  const int bx = cvt_i32(flx), by = cvt_i32(fly), bz = cvt_i32(flz);
  const float fx = pos.x - flx, fy = pos.y - fly, fz = pos.z - flz;
  const int hi = m.size - 1;
  int X[4], Y[4], Z[4];
  se_stencil4(bx, hi, X); se_stencil4(by, hi, Y); se_stencil4(bz, hi, Z);
  const int xb0 = X[0] >> 3, yb0 = Y[0] >> 3, zb0 = Z[0] >> 3;
  const int xb1 = X[3] >> 3, yb1 = Y[3] >> 3, zb1 = Z[3] >> 3;
  // phase 1: entries of the 2x2x2 candidate blocks (coincident ones are the same cache line)
  uint32_t e[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) e[k] = se_block_entry<DENSE>(m, (k & 1) ? xb1 : xb0, (k & 2) ? yb1 : yb0, (k & 4) ? zb1 : zb0, c);
  // phase 2: the 32 voxels.  A voxel's block among the 2x2x2 candidates is (x block != xb0, y block != yb0, z block != zb0): the brick base is
  // picked axis by axis (x: 16 selects, y: 32, z: one per voxel; r04 -- seven compares and selects per voxel before) and the offset inside the
  // brick is a sum of per-axis terms.  `base` = brick offset + 1 in voxels' units (0: no brick), so that "missing" stays one test.
  bool ux[4], uy[4], uz[4];
  uint32_t ox[4], oy[4], oz[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ux[i] = (X[i] >> 3) != xb0; uy[i] = (Y[i] >> 3) != yb0; uz[i] = (Z[i] >> 3) != zb0;
    ox[i] = (uint32_t)X[i] & 7u; oy[i] = ((uint32_t)Y[i] & 7u) << 3; oz[i] = ((uint32_t)Z[i] & 7u) << 6;
  }
  uint32_t ex[4][4];        // [xi][q]: entry of x-voxel xi in the (y, z) block pair q
#pragma unroll
  for (int xi = 0; xi < 4; ++xi)
#pragma unroll
    for (int q = 0; q < 4; ++q) ex[xi][q] = ux[xi] ? e[2 * q + 1] : e[2 * q];
  float V[4][4][4];
#pragma unroll
  for (int yi = 0; yi < 4; ++yi)
#pragma unroll
    for (int xi = 0; xi < 4; ++xi) {
      if (!((xi == 1 || xi == 2) || (yi == 1 || yi == 2))) continue;      // (no voxel of this column is needed)
      const uint32_t exy0 = uy[yi] ? ex[xi][1] : ex[xi][0], exy1 = uy[yi] ? ex[xi][3] : ex[xi][2];
      const uint32_t oxy = ox[xi] + oy[yi];
#pragma unroll
      for (int zi = 0; zi < 4; ++zi) {
        const int central = (xi == 1 || xi == 2) + (yi == 1 || yi == 2) + (zi == 1 || zi == 2);
        if (central < 2) continue;
        const uint32_t ek = uz[zi] ? exy1 : exy0;
        const size_t vi = ek ? (size_t)(ek - 1u) * SE_BRICK_STRIDE + (size_t)(oxy + oz[zi]) : 0;
        const float v = m.vx[vi];
        V[zi][yi][xi] = ek ? v : fc.init_x;
      }
    }
  return se_grad_blend(V, fx, fy, fz);
}

// Octree::grad for a stencil that leaves the volume: every one of the 32 voxels is looked up on its own.  Same clamps, same blend.
__device__ __forceinline__ f3 se_grad_checked(const DevMap& m, const FieldConst fc, f3 pos) {
  const float flx = floorf(pos.x), fly = floorf(pos.y), flz = floorf(pos.z);
  const int bx = cvt_i32(flx), by = cvt_i32(fly), bz = cvt_i32(flz);
  const float fx = pos.x - flx, fy = pos.y - fly, fz = pos.z - flz;
  const int hi = m.size - 1;
  int X[4], Y[4], Z[4];
  se_stencil4(bx, hi, X); se_stencil4(by, hi, Y); se_stencil4(bz, hi, Z);
  float V[4][4][4];
#pragma unroll
  for (int zi = 0; zi < 4; ++zi)
#pragma unroll
    for (int yi = 0; yi < 4; ++yi)
#pragma unroll
      for (int xi = 0; xi < 4; ++xi) {
        const int central = (xi == 1 || xi == 2) + (yi == 1 || yi == 2) + (zi == 1 || zi == 2);
        if (central < 2) continue;
        const int x = X[xi], y = Y[yi], z = Z[zi];
        const uint32_t e = in_volume(m, x, y, z) ? se_query_block(m, x >> 3, y >> 3, z >> 3) : 0u;
        V[zi][yi][xi] = e ? m.vx[se_voxel_index(e, x, y, z)] : fc.init_x;
      }
  return se_grad_blend(V, fx, fy, fz);
}

// ---- the dense grid by per-axis terms (r04) ------------------------------------------------------------------------------------------------------
// The voxel index (bz << 2l | by << l | bx) * 1024 + (x & 7) + 8 (y & 7) + 64 (z & 7) is a sum of one term per axis, (block part << 10) | local part, so
// a sample costs ~4 integer operations per axis and the 8 / 32 voxels of interp / grad one 3-input add each, instead of a full index computation
// per sample (the gradient's 32 samples were a quarter of the raycast's vector instructions).  Maps of <= 4 GiB (O32: 512^3 dense) carry the terms as
// byte offsets and load through a 32-bit offset from the scalar base, the brick's y plane with an immediate offset from the same address
// (y = x + 512 floats, se_device.h).  "Inside the volume" is one compare of the OR of the three integers (size is a power of two, a negative or
// saturated value has high bits set).  Same loads, same arithmetic on the values as the generic forms.
template <bool O32> struct SeDense;
template <> struct SeDense<true> {     // byte-offset terms, 32 bit
  typedef uint32_t idx_t;
  static __device__ __forceinline__ idx_t tx(const DevMap&, uint32_t x) { return ((x >> 3) << 12) | ((x & 7u) << 2); }
  static __device__ __forceinline__ idx_t ty(const DevMap& m, uint32_t y) { return ((y >> 3) << (12 + m.leaf_level)) | ((y & 7u) << 5); }
  static __device__ __forceinline__ idx_t tz(const DevMap& m, uint32_t z) { return ((z >> 3) << (12 + 2 * m.leaf_level)) | ((z & 7u) << 8); }
  static __device__ __forceinline__ idx_t sum(idx_t a, idx_t b, idx_t c) { return a + b + c; }
  static __device__ __forceinline__ float ldx(const DevMap& m, idx_t i) { return *(const float*)((const char*)m.vx + (size_t)i); }
  static __device__ __forceinline__ float ldy(const DevMap& m, idx_t i) { return *(const float*)((const char*)m.vx + (size_t)i + 2048); }
  // SDF: the weight is a byte, 2048 + voxel bytes into the brick (se_device.h)
  static __device__ __forceinline__ float ldyb(const DevMap& m, idx_t i) { return (float)*((const uint8_t*)m.vx + (size_t)((i & 0xFFFFF000u) + 2048u + SE_YB((i >> 2) & 511u))); }
};
template <> struct SeDense<false> {    // (block sum, local sum) in 32 bit each, widened at the load
  struct idx_t { uint32_t blk, loc; };
  static __device__ __forceinline__ idx_t tx(const DevMap&, uint32_t x) { return {x >> 3, x & 7u}; }
  static __device__ __forceinline__ idx_t ty(const DevMap& m, uint32_t y) { return {(y >> 3) << m.leaf_level, (y & 7u) << 3}; }
  static __device__ __forceinline__ idx_t tz(const DevMap& m, uint32_t z) { return {(z >> 3) << (2 * m.leaf_level), (z & 7u) << 6}; }
  static __device__ __forceinline__ idx_t sum(idx_t a, idx_t b, idx_t c) { return {a.blk + b.blk + c.blk, a.loc + b.loc + c.loc}; }
  static __device__ __forceinline__ float ldx(const DevMap& m, idx_t i) { return m.vx[((size_t)i.blk << 10) | i.loc]; }
  static __device__ __forceinline__ float ldy(const DevMap& m, idx_t i) { return m.vx[(((size_t)i.blk << 10) | i.loc) + 512]; }
  static __device__ __forceinline__ float ldyb(const DevMap& m, idx_t i) { return (float)*((const uint8_t*)m.vx + (((size_t)i.blk << 12) + 2048u + SE_YB(i.loc))); }
};
template <bool O32> struct SeCell { float fx, fy, fz; typename SeDense<O32>::idx_t vi[8]; bool inside; };
// the interpolation cell of a point given in voxel units (Octree::interp, octree.hpp:541-563): fractions and the eight
// corner indices; inside = the whole cell lies in the volume (else the caller takes se_interp_generic)
template <bool O32>
__device__ __forceinline__ SeCell<O32> se_cell_lean(const DevMap& m, f3 pos) {
  typedef SeDense<O32> A;
  SeCell<O32> cell;
  const float flx = floorf(pos.x), fly = floorf(pos.y), flz = floorf(pos.z);
  const int bx = se_cvt_hw(flx), by = se_cvt_hw(fly), bz = se_cvt_hw(flz);
  cell.fx = pos.x - flx; cell.fy = pos.y - fly; cell.fz = pos.z - flz;
  const int lx = max(bx, 0), ly = max(by, 0), lz = max(bz, 0);
  const int top = m.size - 1;
  cell.inside = max(max(lx, ly), lz) < top;
  const typename A::idx_t X[2] = {A::tx(m, lx), A::tx(m, lx + 1)}, Y[2] = {A::ty(m, ly), A::ty(m, ly + 1)}, Z[2] = {A::tz(m, lz), A::tz(m, lz + 1)};
#pragma unroll
  for (int k = 0; k < 8; ++k) cell.vi[k] = A::sum(X[k & 1], Y[(k >> 1) & 1], Z[k >> 2]);
  return cell;
}
template <bool O32>
__device__ __forceinline__ float se_interp_lean(const DevMap& m, const FieldConst fc, f3 pos, BlkCache& c) {
  const SeCell<O32> cell = se_cell_lean<O32>(m, pos);
  if (!cell.inside) return se_interp_generic<true>(m, fc, pos, c);   // a corner outside the volume
  float p[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) p[k] = SeDense<O32>::ldx(m, cell.vi[k]);
  return se_trilerp(p, cell.fx, cell.fy, cell.fz);
}
template <bool O32>
__device__ __forceinline__ f3 se_grad_lean(const DevMap& m, const FieldConst fc, f3 pos, BlkCache& c) {
  typedef SeDense<O32> A;
  const float flx = floorf(pos.x), fly = floorf(pos.y), flz = floorf(pos.z);
  const int bx = se_cvt_hw(flx), by = se_cvt_hw(fly), bz = se_cvt_hw(flz);
  const int hi = m.size - 1;
  // indices 0, 1 are clamped from below only (octree.hpp:658-663): they leave the volume when the point does
  if (!(bx <= hi && by <= hi && bz <= hi)) return se_grad_generic<true>(m, fc, pos, c);
  const float fx = pos.x - flx, fy = pos.y - fly, fz = pos.z - flz;
  const typename A::idx_t TX[4] = {A::tx(m, se_stencil(bx, hi, 0)), A::tx(m, se_stencil(bx, hi, 1)), A::tx(m, se_stencil(bx, hi, 2)), A::tx(m, se_stencil(bx, hi, 3))};
  const typename A::idx_t TY[4] = {A::ty(m, se_stencil(by, hi, 0)), A::ty(m, se_stencil(by, hi, 1)), A::ty(m, se_stencil(by, hi, 2)), A::ty(m, se_stencil(by, hi, 3))};
  const typename A::idx_t TZ[4] = {A::tz(m, se_stencil(bz, hi, 0)), A::tz(m, se_stencil(bz, hi, 1)), A::tz(m, se_stencil(bz, hi, 2)), A::tz(m, se_stencil(bz, hi, 3))};
  float V[4][4][4];
#pragma unroll
  for (int zi = 0; zi < 4; ++zi)
#pragma unroll
    for (int yi = 0; yi < 4; ++yi)
#pragma unroll
      for (int xi = 0; xi < 4; ++xi) {
        const int central = (xi == 1 || xi == 2) + (yi == 1 || yi == 2) + (zi == 1 || zi == 2);
        if (central < 2) continue;
        V[zi][yi][xi] = A::ldx(m, A::sum(TX[xi], TY[yi], TZ[zi]));
      }
  return se_grad_blend(V, fx, fy, fz);
}

// interp / grad for a caller that knows the layout only as dense or pooled (the point query): on the dense grid the lean forms with (block, local)
// terms, which hold for every map size, else the generic ones.
// (Kept as a level of their own on purpose: with the generic forms called directly the pooled raycast kernels and k_query_points<false> compile
// differently, profiles/march_fold_asm.txt.  se_hit_grad calls se_grad_lean<O32> directly for the same reason.)
template <bool DENSE>
__device__ __forceinline__ float se_interp(const DevMap& m, const FieldConst fc, f3 pos, BlkCache& c) {
  if (!DENSE) return se_interp_generic<DENSE>(m, fc, pos, c);
  return se_interp_lean<false>(m, fc, pos, c);
}
template <bool DENSE>
__device__ __forceinline__ f3 se_grad(const DevMap& m, const FieldConst fc, f3 pos, BlkCache& c) {
  if (!DENSE) return se_grad_generic<DENSE>(m, fc, pos, c);
  return se_grad_lean<false>(m, fc, pos, c);
}

// The normal at a hit (raycastKernel / renderVolumeKernel: volume.grad(hit)).  A hit can lie up to a voxel beyond an upper face of the volume
// (floor(q) = size: the reference's `lower` index max(base, 0) is not clamped there and reads initValue()), outside the band; there every voxel
// of the stencil is read by itself.  (Seen from beyond the +x / +y / +z faces, tests/test_gpu_beam_shell.py.)
template <bool DENSE, bool O32 = false>
__device__ __forceinline__ f3 se_hit_grad(const DevMap& m, const FieldConst fc, f3 q, BlkCache& c) {
  const int hi = m.size - 1;
  const int bx = cvt_i32(floorf(q.x)), by = cvt_i32(floorf(q.y)), bz = cvt_i32(floorf(q.z));
  if (!SE_GRAD_BAND(bx, by, bz, hi)) return se_grad_checked(m, fc, q);
  return DENSE ? se_grad_lean<O32>(m, fc, q, c) : se_grad<DENSE>(m, fc, q, c);
}

// one get() on the dense grid: inside-the-volume flag and index of the sample at q (metres; inv_voxel = size / dim)
template <bool O32> struct SeSample { typename SeDense<O32>::idx_t vi; bool in; };
template <bool O32>
__device__ __forceinline__ SeSample<O32> se_sample_lean(const DevMap& m, float inv_voxel, f3 q) {
  typedef SeDense<O32> A;
  const int ix = se_cvt_hw(inv_voxel * q.x), iy = se_cvt_hw(inv_voxel * q.y), iz = se_cvt_hw(inv_voxel * q.z);
  SeSample<O32> s;
  s.in = (uint32_t)(ix | iy | iz) < (uint32_t)m.size;
  const uint32_t ux = s.in ? (uint32_t)ix : 0u, uy = s.in ? (uint32_t)iy : 0u, uz = s.in ? (uint32_t)iz : 0u;   // (outside: voxel 0, value replaced)
  s.vi = A::sum(A::tx(m, ux), A::ty(m, uy), A::tz(m, uz));
  return s;
}
// ---- the same for pooled bricks (the north-star layout: bump-allocated bricks behind the index).  A sample's block entry comes from
// tab[]; while the march is in unobserved space (`unobs`) it asks the leaf bitmap first, so that a block that was never allocated costs a bit test
// in an L2-resident array instead of a line of the 8 / 64 MB leaf index.  The entry of the previous sample's block is kept (most steps
// stay in or next to it).  interp / grad of a hit go through the generic forms (eight / 2x2x2 block look-ups).
struct SePSample { uint32_t e, loc; int bx, by, bz; };
struct SePCache { uint32_t lin, e; };
__device__ __forceinline__ SePSample se_sample_pooled(const DevMap& m, float inv_voxel, f3 q, SePCache& c, bool unobs) {
  const int ix = se_cvt_hw(inv_voxel * q.x), iy = se_cvt_hw(inv_voxel * q.y), iz = se_cvt_hw(inv_voxel * q.z);
  const bool in = (uint32_t)(ix | iy | iz) < (uint32_t)m.size;
  SePSample s;
  s.bx = ix >> 3; s.by = iy >> 3; s.bz = iz >> 3;
  s.loc = ((uint32_t)ix & 7u) | (((uint32_t)iy & 7u) << 3) | (((uint32_t)iz & 7u) << 6);
  s.e = 0u;
  if (in) {
    const uint32_t lin = block_linear(m, s.bx, s.by, s.bz);
    if (lin == c.lin) s.e = c.e;
    else {
      bool present = true;
      if (unobs) present = (m.lbits[lin >> 5] >> (lin & 31u)) & 1u;
      uint32_t e = 0u;
      if (present) { e = m.tab[m.leaf_off + lin]; e = e == SE_PENDING ? 0u : e; }   // (PENDING: see se_block_entry)
      c.lin = lin; c.e = e;
      s.e = e;
    }
  }
  return s;
}
__device__ __forceinline__ size_t se_pooled_index(const SePSample& s) { return ((size_t)(s.e ? s.e - 1u : 0u) << 10) | s.loc; }
