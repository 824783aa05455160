// Batched point queries against the resident map (se_hip_query_points, include/se_hip.h): for N points in metres, what the
// reference's map read interface VolumeTemplate (se_denseslam/include/se/continuous/volume_template.hpp:77-102) answers --
// get(p) = Octree::get_fine, operator[](p) = Octree::get (coarse node value where no block exists), interp(p, x) and grad(p, x).
//
// One thread per point, grid-stride loop over int64 n, wave64 workgroups.  interp / grad are the raycast's own inline
// forms of se_sample.h (bit-exact with Octree::interp / Octree::grad); the coarse walk is the index pyramid read top-down.
// Voxel coordinates: q = s * p per axis (s = (float)size / dim), v = (int)q (truncation, VolumeTemplate::get / operator[]).
// A point with a non-finite q or |q| >= 2^20 on any axis gets the defaults (status 0, initValue() for fine and coarse,
// empty().x for interp, 0 for grad) and touches no map memory; see se_hip.h for the full definition of every output.
#pragma once
#include "se_kernels.h"

#define SE_WG_QUERY 64           // one wave per workgroup
#define SE_QUERY_LIMIT 1048576.f // |s * p| below 2^20 on every axis, else the point is refused (status 0)

// status bits of se_hip_query_out::status
#define SE_Q_IN_VOLUME 1u        // v lies in [0, size)^3
#define SE_Q_ALLOCATED 2u        // the block holding v is allocated
#define SE_Q_OBSERVED 4u         // all eight voxels interp reads lie in allocated blocks

struct QueryOut { float* fine; float* coarse; float* interp; float* grad; uint8_t* status; };

// One instantiation per brick layout.  The field type needs none: y is read through se_ld_y, whose byte / float plane test is uniform
// across the wave, and initValue() / empty() come from the map (FieldConst).
template <bool DENSE>
__global__ __launch_bounds__(SE_WG_QUERY) void k_query_points(DevMap m, const float* __restrict__ pts, long long n, QueryOut o, float s, float grad_scale) {
  const FieldConst fc = se_field_const(m);
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const f3 q = {s * pts[3 * i], s * pts[3 * i + 1], s * pts[3 * i + 2]};
    float fine_x = fc.init_x, fine_y = fc.init_y, coarse_x = fc.init_x, coarse_y = fc.init_y, ip = fc.empty_x;
    f3 g = {0.f, 0.f, 0.f};
    uint32_t st = 0u;
    // (a NaN fails every comparison)
    if (fabsf(q.x) < SE_QUERY_LIMIT && fabsf(q.y) < SE_QUERY_LIMIT && fabsf(q.z) < SE_QUERY_LIMIT) {
      const int x = cvt_i32(q.x), y = cvt_i32(q.y), z = cvt_i32(q.z);
      if (in_volume(m, x, y, z)) {
        st |= SE_Q_IN_VOLUME;
        const uint32_t e = se_query_block(m, x >> 3, y >> 3, z >> 3);
        if (e) {
          st |= SE_Q_ALLOCATED;
          const size_t vi = se_voxel_index(e, x, y, z);
          fine_x = coarse_x = m.vx[vi];
          fine_y = coarse_y = se_ld_y(m, vi);
        } else if (o.coarse) {
          int sh;   // Octree::get: the value of the first missing octant on the block's path (absent_value_slot, se_device.h)
          const size_t vs = absent_value_slot(m, x >> 3, y >> 3, z >> 3, sh);
          coarse_x = m.nx[vs];
          coarse_y = m.ny[vs];
        }
      }
      if (o.status) {
        // the interpolation cell of se_interp_generic / Octree::interp: corners lower .. lower + 1 per axis, lower = max(floor(q), 0)
        const int lx = max(cvt_i32(floorf(q.x)), 0), ly = max(cvt_i32(floorf(q.y)), 0), lz = max(cvt_i32(floorf(q.z)), 0);
        const bool cx = (lx & 7) == 7, cy = (ly & 7) == 7, cz = (lz & 7) == 7;
        bool all = true;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const bool need = (!(k & 1) || cx) && (!(k & 2) || cy) && (!(k & 4) || cz);
          if (need && all) all = se_query_block(m, (lx + (k & 1)) >> 3, (ly + ((k >> 1) & 1)) >> 3, (lz + (k >> 2)) >> 3) != 0u;
        }
        st |= all ? SE_Q_OBSERVED : 0u;
      }
      BlkCache c = {-1, -1, -1, 0u};
      // On the dense grid se_interp / se_grad are the lean forms, which convert float -> int with the hardware instruction (se_cvt_hw) where the generic
      // ones convert as cvttss2si does (cvt_i32): the two agree for non-NaN |f| < 2^31, and |q| < SE_QUERY_LIMIT = 2^20 on every axis here.
      if (o.interp) ip = se_interp<DENSE>(m, fc, q, c);
      if (o.grad) {
        const int hi = m.size - 1;
        const int bx = cvt_i32(floorf(q.x)), by = cvt_i32(floorf(q.y)), bz = cvt_i32(floorf(q.z));
        const bool band = SE_GRAD_BAND(bx, by, bz, hi);   // outside it se_grad_checked reads each voxel by itself (se_sample.h)
        g = f3_scale(grad_scale, band ? se_grad<DENSE>(m, fc, q, c) : se_grad_checked(m, fc, q));
      }
    }
    if (o.fine) { o.fine[2 * i] = fine_x; o.fine[2 * i + 1] = fine_y; }
    if (o.coarse) { o.coarse[2 * i] = coarse_x; o.coarse[2 * i + 1] = coarse_y; }
    if (o.interp) o.interp[i] = ip;
    if (o.grad) { o.grad[3 * i] = g.x; o.grad[3 * i + 1] = g.y; o.grad[3 * i + 2] = g.z; }
    if (o.status) o.status[i] = (uint8_t)st;
  }
}
