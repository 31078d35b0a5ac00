// f2: the exact (erf) GELU of Swin's MLP as elementwise kernels, for the training path of
// HipSwinLayer: with gradients fc1 stores its pre-activation u (act none) and
//   m  = gelu(u)            = 0.5 u (1 + erf(u / sqrt 2))       the formula of gemm.hip's g_act
//   du = dm * gelu'(u),  gelu'(u) = 0.5 (1 + erf(u / sqrt 2)) + u exp(-u^2 / 2) / sqrt(2 pi)
// Float32 arithmetic, one rounding to the operand dtype; 8 elements per thread (two 16-byte
// accesses in f32, one in bf16), the tail element by element.  Bound: HBM (2 / 3 streams).
#include "common.hpp"

namespace rgbd {
namespace {

__device__ __forceinline__ float gelu_f(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_df(float v) {
  return 0.5f * (1.f + erff(v * 0.70710678118654752f)) + v * expf(-0.5f * v * v) * 0.39894228040143268f;
}

template <typename T, bool BWD>
__global__ __launch_bounds__(256) void k_gelu(const T* __restrict__ u, const T* __restrict__ dm, T* __restrict__ out,
                                              long long n) {
  const long long i0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 8;
  if (i0 >= n) return;
  if (i0 + 8 <= n) {
    T uu[8], dd[8], oo[8];
    __builtin_memcpy(uu, __builtin_assume_aligned(u + i0, 16), sizeof(uu));
    if (BWD) __builtin_memcpy(dd, __builtin_assume_aligned(dm + i0, 16), sizeof(dd));
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float x = Num<T>::to_f(uu[j]);
      oo[j] = Num<T>::from_f(BWD ? Num<T>::to_f(dd[j]) * gelu_df(x) : gelu_f(x));
    }
    __builtin_memcpy(__builtin_assume_aligned(out + i0, 16), oo, sizeof(oo));
  } else {
    for (long long i = i0; i < n; ++i) {
      const float x = Num<T>::to_f(u[i]);
      out[i] = Num<T>::from_f(BWD ? Num<T>::to_f(dm[i]) * gelu_df(x) : gelu_f(x));
    }
  }
}

template <bool BWD>
int launch(int dtype, const void* u, const void* dm, void* out, long long n, void* stream) {
  RGBD_REQUIRE(n >= 0, RGBD_E_ARG);
  if (n == 0) return RGBD_OK;
  RGBD_REQUIRE(u && out && (!BWD || dm), RGBD_E_ARG);
  RGBD_REQUIRE(dtype == RGBD_BF16 || dtype == RGBD_F32, RGBD_E_DTYPE);
  RGBD_REQUIRE(((uintptr_t)u | (uintptr_t)out | (uintptr_t)dm) % 16 == 0, RGBD_E_SHAPE);
  const long long blocks = (n + 2047) / 2048;
  RGBD_REQUIRE(blocks <= 0x7fffffffLL, RGBD_E_SHAPE);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == RGBD_BF16)
    hipLaunchKernelGGL((k_gelu<bf16_t, BWD>), dim3((unsigned)blocks), dim3(256), 0, s, (const bf16_t*)u,
                       (const bf16_t*)dm, (bf16_t*)out, n);
  else
    hipLaunchKernelGGL((k_gelu<float, BWD>), dim3((unsigned)blocks), dim3(256), 0, s, (const float*)u,
                       (const float*)dm, (float*)out, n);
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

}  // namespace
}  // namespace rgbd

extern "C" {

int rgbd_gelu(int dtype, const void* u, void* m, long long n, void* stream) {
  return rgbd::launch<false>(dtype, u, nullptr, m, n, stream);
}

int rgbd_gelu_bwd(int dtype, const void* u, const void* dm, void* du, long long n, void* stream) {
  return rgbd::launch<true>(dtype, u, dm, du, n, stream);
}

}  // extern "C"
