// TEST INFRASTRUCTURE (never part of the product path): the CPU side of the batched ray casts (se_hip_cast_rays, include/se_hip.h) on the
// oracle's pipeline (oracle/se_oracle.cpp Pipeline<VT>, created through so_pipe_create of this same library).
//   rco_camera_rays  the [W * H][8] rays of the oracle's raycastKernel (se_denseslam/src/rendering.cpp:51-90) for pose * K^-1:
//                    origin = the view's translation, direction = normalized(top3(view) * (x, y, 1)), near / far = 0.4 / 4.0.
//   rco_cast_rays    the per-pixel body of raycastKernel for each ray of the caller's (RayIterator from its origin along its direction
//                    within [near, far], raycast() from t_min if t_min > 0, grad at a hit), plus the header's rules for invalid rays and
//                    its status bits.  Returns the largest number of iterator trips any ray took (the device search stops at 4096).
#include "../../oracle/se_oracle.cpp"

namespace rco {

constexpr float kOriginLimit = 1048576.f;   // |s * o| < 2^20, s = (float)size / dim
constexpr float kDirMin = 0.98f, kDirMax = 1.02f;

template <typename VT>
static int cast(Pipeline<VT>* P, const float* rays, long long n, float mu, float* hit, float* normal, uint8_t* status) {
  Volume<VT> volume = P->volume;
  volume.st = nullptr;
  const float step = volume._dim / volume._size;   // DenseSLAMSystem.cpp:197
  const float largestep = step * BLOCK_SIDE;
  const float s = (float)volume._size / volume._dim;
  int max_trips = 0;
#pragma omp parallel for reduction(max : max_trips) schedule(dynamic, 256)
  for (long long i = 0; i < n; ++i) {
    const float* q = rays + 8 * i;
    const V3f o = {q[0], q[1], q[2]}, d = {q[3], q[4], q[5]};
    const float nearp = q[6], farp = q[7];
    const float dd = (d.x * d.x + d.y * d.y) + d.z * d.z;
    const bool valid = std::fabs(s * o.x) < kOriginLimit && std::fabs(s * o.y) < kOriginLimit && std::fabs(s * o.z) < kOriginLimit &&
                       dd >= kDirMin && dd <= kDirMax && std::isfinite(nearp) && std::isfinite(farp);
    V4f h = {0.f, 0.f, 0.f, 0.f};
    V3f nn = {INVALID, 0.f, 0.f};
    uint8_t st = 0;
    if (valid) {
      st = 1;
      g_ray_iter = g_ray_get = g_ray_interp = 0;
      RayIterator<VT> ray(*volume._map_index, o, d, nearp, farp);
      const bool found = ray.next() != nullptr;
      max_trips = std::max(max_trips, g_ray_iter);
      const float t_min = ray.tcmin();
      if (t_min > 0.f) {
        h = raycast(volume, o, d, t_min, ray.tmax(), mu, step, largestep);
        if (found) st |= 2;
      }
      if (h.w > 0.0) {
        st |= 4;
        const V3f surfNorm = volume.grad({h.x, h.y, h.z});
        if (norm(surfNorm) != 0) {
          st |= 8;
          nn = P->is_sdf ? normalized(-1.f * surfNorm) : normalized(surfNorm);
        }
      }
    }
    if (hit) { hit[4 * i] = h.x; hit[4 * i + 1] = h.y; hit[4 * i + 2] = h.z; hit[4 * i + 3] = h.w; }
    if (normal) { normal[3 * i] = nn.x; normal[3 * i + 1] = nn.y; normal[3 * i + 2] = nn.z; }
    if (status) status[i] = st;
  }
  return max_trips;
}

}  // namespace rco

extern "C" void rco_camera_rays(const float* pose_cm, const float* k, int W, int H, float* out) {
  const M4 view = mul(from_colmajor(pose_cm), inverse_camera_matrix(k));   // DenseSLAMSystem.cpp:199
  const V3f transl = {view.m[0][3], view.m[1][3], view.m[2][3]};
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const V3f dir = normalized(mul3(top3(view), {(float)x, (float)y, 1.f}));
      float* r = out + 8 * ((size_t)x + (size_t)y * W);
      r[0] = transl.x; r[1] = transl.y; r[2] = transl.z;
      r[3] = dir.x; r[4] = dir.y; r[5] = dir.z;
      r[6] = nearPlane; r[7] = farPlane;
    }
}

extern "C" int rco_cast_rays(void* pipe, const float* rays, long long n, float mu, float* hit, float* normal, uint8_t* status) {
  PipelineBase* b = (PipelineBase*)pipe;
  if (auto* s = dynamic_cast<Pipeline<SDFv>*>(b)) return rco::cast(s, rays, n, mu, hit, normal, status);
  if (auto* o = dynamic_cast<Pipeline<OFv>*>(b)) return rco::cast(o, rays, n, mu, hit, normal, status);
  return -1;
}
