// Batched ray casts against the resident map (se_hip_cast_rays, include/se_hip.h): for N rays (origin, direction, near, far in metres),
// exactly the per-pixel body of the reference's raycastKernel (se_denseslam/src/rendering.cpp:51-90) with the ray's own origin, direction
// and planes in place of the camera's -- ray_iterator up to the first leaf, the field's march (kfusion / bfusion rendering_impl.hpp),
// Octree::grad at the hit.
//
// One thread per ray, SE_WG_RAY threads per workgroup (se_first_leaf indexes its LDS stack by threadIdx.x).  The workgroup stages the
// occupancy levels 1..cache_levels in LDS once, as se_raycast_wg does; every thread, the tail past n included, reaches that barrier before
// any per-ray branch, and there is no barrier after it.  Then each thread runs the full stack iterator se_first_leaf from its own near
// plane (no beam start: the rays are not a tile), se_cast_ray and se_hit_grad -- the camera raycast's own inline functions, unchanged.
// The per-ray quantities the camera path forms once on the host (origin / dim + 1, near / dim, far / dim) are formed here with the same
// float operations, in a local copy of RayArgs.  The loops are the iterator's trip cap and the march, which step > 0 and the direction
// band bound.  A ray with a non-finite value, |s * o| >= 2^20 on an axis or a direction outside the band gets the miss outputs and status 0
// without reading the map.
#pragma once
#include "se_kernels.h"

#define SE_RAY_ORIGIN_LIMIT 1048576.f   // |s * o| below 2^20 on every axis (s = size / dim), the limit of the point queries
#define SE_RAY_DIR_MIN 0.98f            // squared norm of the direction, (dx * dx + dy * dy) + dz * dz, within [MIN, MAX]
#define SE_RAY_DIR_MAX 1.02f
#define SE_RAY_MAX_LAUNCH (1ll << 24)   // rays per launch; the host splits larger batches

// status bits of se_hip_ray_out::status
#define SE_R_VALID 1u     // the ray passed the checks above
#define SE_R_ENTERED 2u   // the iterator returned an allocated block at t_min > 0: the march ran
#define SE_R_HIT 4u       // the march returned w > 0
#define SE_R_NORMAL 8u    // the gradient at the hit is not zero

struct CastRayOut { float* hit; float* normal; uint8_t* status; };

template <bool OFUSION, bool DENSE, bool SHALLOW, bool O32>
__global__ __launch_bounds__(SE_WG_RAY) void k_cast_rays(DevMap m, RayArgs a, const float* __restrict__ rays, long long n, CastRayOut o, float s) {
  extern __shared__ uint32_t smem[];
  // LDS: [occupancy words of levels 1..cache_levels][ray stack: parent codes][ray stack: t_max] (the layout of se_raycast_wg)
  uint32_t* s_occ = smem;
  uint32_t* s_par = smem + a.cache_words;
  float* s_tmax = (float*)(s_par + a.stack_depth * SE_WG_RAY);
  for (int i = threadIdx.x; i < a.cache_words; i += SE_WG_RAY) s_occ[i] = m.occ[i];
  __syncthreads();
  const long long r = (long long)blockIdx.x * SE_WG_RAY + threadIdx.x;
  if (r >= n) return;
  const float* q = rays + 8 * r;
  const f3 org = {q[0], q[1], q[2]}, dir = {q[3], q[4], q[5]};
  const float nearp = q[6], farp = q[7];
  const float dd = (dir.x * dir.x + dir.y * dir.y) + dir.z * dir.z;
  // (a NaN fails every comparison; an infinite near / far fails the finiteness test)
  const bool valid = fabsf(s * org.x) < SE_RAY_ORIGIN_LIMIT && fabsf(s * org.y) < SE_RAY_ORIGIN_LIMIT && fabsf(s * org.z) < SE_RAY_ORIGIN_LIMIT &&
                     dd >= SE_RAY_DIR_MIN && dd <= SE_RAY_DIR_MAX && __builtin_isfinite(nearp) && __builtin_isfinite(farp);
  float hx = 0.f, hy = 0.f, hz = 0.f, hw = 0.f;
  f3 nn = {-2.f, 0.f, 0.f};   // INVALID (commons.h:71)
  uint32_t st = 0u;
  if (valid) {
    st = SE_R_VALID;
    RayArgs ra = a;
    ra.scaled_origin[0] = org.x / m.dim + 1.f;   // ray_iterator.hpp:79
    ra.scaled_origin[1] = org.y / m.dim + 1.f;
    ra.scaled_origin[2] = org.z / m.dim + 1.f;
    ra.near_n = nearp / m.dim;                   // ray_iterator.hpp:101-102
    ra.far_n = farp / m.dim;
    const RaySpan span = se_first_leaf<SHALLOW>(m, ra, org, dir, s_occ, s_par, s_tmax);
    const FieldConst fc = se_field_const(m);
    BlkCache c = {-1, -1, -1, 0u};
    if (span.tcmin > 0.f) {
      RayCounters rc = {0ull, 0ull, 0u};
      se_cast_ray<OFUSION, false, DENSE, O32>(m, ra, fc, org, dir, span.tcmin, span.tmax, c, hx, hy, hz, hw, rc);
      if (span.found) st |= SE_R_ENTERED;
    }
    if (hw > 0.f) {   // (hit.w() > 0.0)
      st |= SE_R_HIT;
      const f3 g = se_hit_grad<DENSE, O32>(m, fc, f3_scale(a.inv_voxel, {hx, hy, hz}), c);
      const f3 surfNorm = f3_scale(a.grad_scale, g);
      if (sqrtf(f3_sqnorm(surfNorm)) != 0) {
        st |= SE_R_NORMAL;
        nn = OFUSION ? f3_normalized(surfNorm) : f3_normalized(f3_scale(-1.f, surfNorm));
      }
    }
  }
  // hit: the V4f the march returned ({0, 0, 0, 0} unless it found a crossing)
  if (o.hit) { float* h = o.hit + 4 * r; h[0] = hx; h[1] = hy; h[2] = hz; h[3] = hw; }
  if (o.normal) { float* v = o.normal + 3 * r; v[0] = nn.x; v[1] = nn.y; v[2] = nn.z; }
  if (o.status) o.status[r] = (uint8_t)st;
}
