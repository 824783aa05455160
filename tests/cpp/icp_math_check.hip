// TEST INFRASTRUCTURE (not part of the product library): the scalar core of the device-resident ICP -- se_sincos_f32, se_solve6_wave and
// se_icp_finalize, and the bilateral filter's se_exp_f32, of supereight_amd/csrc/se_track_kernels.h, the production functions themselves -- run on argument lists of the caller's
// choice, so that tests/test_gpu_icp_math.py can compare them with the oracle where no scene takes them.
// Built on demand by that test with the library's own flags.  Every pointer of the entries is a host pointer.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../supereight_amd/csrc/se_track_kernels.h"

namespace {
__global__ void k_chk_sincos(const float* __restrict__ x, int n, float* __restrict__ s, float* __restrict__ c) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) se_sincos_f32(x[i], s + i, c + i);
}
__global__ void k_chk_exp(const float* __restrict__ x, int n, float* __restrict__ e) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) e[i] = se_exp_f32(x[i]);
}

// one wave per system: the 27 values go to LDS (where k_icp_iter keeps them), x[6] comes out of lane 0; agree = every lane holds the same x
__global__ __launch_bounds__(64) void k_chk_solve6(const float* __restrict__ vals, float* __restrict__ x6, int* __restrict__ agree) {
  __shared__ float v[27];
  const int t = threadIdx.x;
  if (t < 27) v[t] = vals[27 * (size_t)blockIdx.x + t];
  __syncthreads();
  float x[6];
  se_solve6_wave(v, x, t);
  bool same = true;
#pragma unroll
  for (int i = 0; i < 6; ++i) same = same && __float_as_uint(x[i]) == __float_as_uint(se_lane(x[i], 0));
  const int all_same = __all(same);
  if (t == 0) {
#pragma unroll
    for (int i = 0; i < 6; ++i) x6[6 * (size_t)blockIdx.x + i] = x[i];
    agree[blockIdx.x] = all_same;
  }
}

// one workgroup of SE_TRACK_LANES per case: a block of partial rows [8][SE_TRACK_SEGMENTS][32], the pose it tracked with, icp_threshold
__global__ __launch_bounds__(SE_TRACK_LANES) void k_chk_finalize(const float* __restrict__ partial, const float* __restrict__ pose, const float* __restrict__ thr,
                                                                  float* __restrict__ strip0, float* __restrict__ pose_out, int* __restrict__ conv) {
  __shared__ IcpShared sh;
  const size_t c = blockIdx.x;
  const int t = threadIdx.x;
  float P[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) P[i] = pose[16 * c + i];
  se_icp_finalize(sh, partial + c * (8 * SE_TRACK_SEGMENTS * 32), P, thr[c]);
  if (t < 32) strip0[32 * c + t] = sh.strip[0][t];
  if (t < 16) pose_out[16 * c + t] = sh.pose[t];
  if (t == 0) conv[c] = sh.conv;
}

struct DevBuf {
  void* p = nullptr;
  bool ok = true;
  DevBuf(size_t bytes, const void* host = nullptr) {
    ok = hipMalloc(&p, bytes ? bytes : 1) == hipSuccess;
    if (ok && host && bytes) ok = hipMemcpy(p, host, bytes, hipMemcpyHostToDevice) == hipSuccess;
  }
  ~DevBuf() { if (p) hipFree(p); }
  bool get(void* host, size_t bytes) const { return hipMemcpy(host, p, bytes, hipMemcpyDeviceToHost) == hipSuccess; }
  template <class T> T* as() const { return static_cast<T*>(p); }
};
int finish() { return (hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess) ? 0 : -2; }
}  // namespace

// Each entry returns 0, or a negative number when a HIP call failed.
extern "C" int se_icp_math_sincos(const float* x, int n, float* s, float* c) {
  if (n <= 0) return 0;
  const size_t bytes = (size_t)n * sizeof(float);
  DevBuf dx(bytes, x), ds(bytes), dc(bytes);
  if (!dx.ok || !ds.ok || !dc.ok) return -1;
  hipLaunchKernelGGL(k_chk_sincos, dim3(2048), dim3(256), 0, 0, dx.as<float>(), n, ds.as<float>(), dc.as<float>());
  if (int r = finish()) return r;
  return ds.get(s, bytes) && dc.get(c, bytes) ? 0 : -3;
}

// se_exp_f32, the bilateral filter's exponential: arguments <= 0 or NaN
extern "C" int se_icp_math_exp(const float* x, int n, float* e) {
  if (n <= 0) return 0;
  const size_t bytes = (size_t)n * sizeof(float);
  DevBuf dx(bytes, x), de(bytes);
  if (!dx.ok || !de.ok) return -1;
  hipLaunchKernelGGL(k_chk_exp, dim3(2048), dim3(256), 0, 0, dx.as<float>(), n, de.as<float>());
  if (int r = finish()) return r;
  return de.get(e, bytes) ? 0 : -3;
}

extern "C" int se_icp_math_solve6(const float* vals27, int n, float* x6, int* agree) {
  if (n <= 0) return 0;
  DevBuf dv((size_t)n * 27 * sizeof(float), vals27), dx((size_t)n * 6 * sizeof(float)), da((size_t)n * sizeof(int));
  if (!dv.ok || !dx.ok || !da.ok) return -1;
  hipLaunchKernelGGL(k_chk_solve6, dim3(n), dim3(64), 0, 0, dv.as<float>(), dx.as<float>(), da.as<int>());
  if (int r = finish()) return r;
  return dx.get(x6, (size_t)n * 6 * sizeof(float)) && da.get(agree, (size_t)n * sizeof(int)) ? 0 : -3;
}

extern "C" int se_icp_math_finalize(const float* partial, const float* pose16, const float* icp_threshold, int n, float* strip0, float* pose_out16, int* conv) {
  if (n <= 0) return 0;
  const size_t block = (size_t)8 * SE_TRACK_SEGMENTS * 32 * sizeof(float);
  DevBuf dp((size_t)n * block, partial), dq((size_t)n * 16 * sizeof(float), pose16), dt((size_t)n * sizeof(float), icp_threshold);
  DevBuf ds((size_t)n * 32 * sizeof(float)), dout((size_t)n * 16 * sizeof(float)), dc((size_t)n * sizeof(int));
  if (!dp.ok || !dq.ok || !dt.ok || !ds.ok || !dout.ok || !dc.ok) return -1;
  hipLaunchKernelGGL(k_chk_finalize, dim3(n), dim3(SE_TRACK_LANES), 0, 0, dp.as<float>(), dq.as<float>(), dt.as<float>(), ds.as<float>(), dout.as<float>(), dc.as<int>());
  if (int r = finish()) return r;
  return ds.get(strip0, (size_t)n * 32 * sizeof(float)) && dout.get(pose_out16, (size_t)n * 16 * sizeof(float)) && dc.get(conv, (size_t)n * sizeof(int)) ? 0 : -3;
}

extern "C" int se_icp_math_segments() { return SE_TRACK_SEGMENTS; }
