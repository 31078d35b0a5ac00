// NCHW -> NHWC layout converters (the channels-last copies the implicit-GEMM kernels read: K5's
// inputs and upstream gradients, the DGGM path's colour maps; color_grad.hip is the inverse), and
// the library's version string.
#include <type_traits>

#include "common.hpp"

using namespace rgbd;

namespace {

template <typename T>
__global__ __launch_bounds__(256) void k_nchw_to_nhwc(const T* __restrict__ src, T* __restrict__ dst, int C,
                                                      int HW) {
  __shared__ T tile[32][33];
  const int b = blockIdx.z;
  const int p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  for (int k = ty; k < 32; k += 8) {
    const int c = c0 + k, p = p0 + tx;
    if (c < C && p < HW) tile[k][tx] = src[((long long)b * C + c) * HW + p];
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) {
    const int p = p0 + k, c = c0 + tx;
    if (c < C && p < HW) dst[((long long)b * HW + p) * C + c] = tile[tx][k];
  }
}

// bf16 NCHW -> NHWC with 16-byte global accesses (HW % 8 == 0, C % 8 == 0): a workgroup moves a
// 64-channel x 64-pixel tile; loads take 8 pixels of one channel, stores 8 channels of one pixel,
// the transpose happens in the LDS writes ([pixel][channel] rows padded to 72 elements).
// Kept beside the one-job case of k_nchw_to_nhwc_multi below, which does the same work: at
// 8 x 96 x 120 x 160 the 3-D grid takes 12.07 us against 12.79 us for the flat grid's index
// arithmetic (profiles/one_kernel_per_op/micro.txt).
__global__ __launch_bounds__(256) void k_nchw_to_nhwc_v8(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst,
                                                         int C, int HW) {
  __shared__ __attribute__((aligned(16))) bf16_t tile[64][72];
  const int b = blockIdx.z, p0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int v = threadIdx.x + 256 * k, cl = v >> 3, pl = (v & 7) * 8;  // channel, 8-pixel group
    const int c = c0 + cl, p = p0 + pl;
    uint4 u = make_uint4(0u, 0u, 0u, 0u);
    if (c < C && p < HW) u = *reinterpret_cast<const uint4*>(src + ((long long)b * C + c) * HW + p);
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      tile[pl + 2 * e][cl] = (bf16_t)(w[e] & 0xffffu);
      tile[pl + 2 * e + 1][cl] = (bf16_t)(w[e] >> 16);
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int v = threadIdx.x + 256 * k, pl = v >> 3, cl = (v & 7) * 8;  // pixel, 8-channel group
    const int p = p0 + pl, c = c0 + cl;
    if (p < HW && c < C)
      *reinterpret_cast<uint4*>(dst + ((long long)b * HW + p) * C + c) = *reinterpret_cast<const uint4*>(&tile[pl][cl]);
  }
}

// Several bf16 NCHW -> NHWC conversions in one launch (the hot path's four colour maps in the
// forward, its three upstream gradients in the backward): a 1-D grid of 64 x 64 tiles over all
// jobs; a job whose HW is not a multiple of 8 loads its pixels one by one (same tile, same stores).
constexpr int NHWC_MAXJOB = 4;
struct NhwcJobs {
  const bf16_t* src[NHWC_MAXJOB];
  bf16_t* dst[NHWC_MAXJOB];
  int C[NHWC_MAXJOB], HW[NHWC_MAXJOB], tp[NHWC_MAXJOB], tc[NHWC_MAXJOB];
  int block0[NHWC_MAXJOB + 1];  // first block of each job; block0[n] = grid
  int n;
};
__global__ __launch_bounds__(256) void k_nchw_to_nhwc_multi(const NhwcJobs J) {
  __shared__ __attribute__((aligned(16))) bf16_t tile[64][72];
  int j = 0;
#pragma unroll
  for (int i = 1; i < NHWC_MAXJOB; ++i)
    if (i < J.n && (int)blockIdx.x >= J.block0[i]) j = i;
  const bf16_t* src = J.src[j];
  bf16_t* dst = J.dst[j];
  const int C = J.C[j], HW = J.HW[j], per = J.tp[j] * J.tc[j];
  const int idx = blockIdx.x - J.block0[j], b = idx / per, t = idx - b * per;
  const int p0 = (t % J.tp[j]) * 64, c0 = (t / J.tp[j]) * 64;
  const bool vec = (HW & 7) == 0;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int v = threadIdx.x + 256 * k, cl = v >> 3, pl = (v & 7) * 8;  // channel, 8-pixel group
    const int c = c0 + cl, p = p0 + pl;
    const bf16_t* row = src + ((long long)b * C + c) * HW;
    bf16_t e8[8];
    if (vec) {
      uint4 u = make_uint4(0u, 0u, 0u, 0u);
      if (c < C && p < HW) u = *reinterpret_cast<const uint4*>(row + p);
      const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        e8[2 * e] = (bf16_t)(w[e] & 0xffffu);
        e8[2 * e + 1] = (bf16_t)(w[e] >> 16);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) e8[e] = (c < C && p + e < HW) ? row[p + e] : (bf16_t)0;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) tile[pl + e][cl] = e8[e];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int v = threadIdx.x + 256 * k, pl = v >> 3, cl = (v & 7) * 8;  // pixel, 8-channel group
    const int p = p0 + pl, c = c0 + cl;
    if (p < HW && c < C)
      *reinterpret_cast<uint4*>(dst + ((long long)b * HW + p) * C + c) = *reinterpret_cast<const uint4*>(&tile[pl][cl]);
  }
}

// The same for float32 sources (the float32-interface bf16 mode: colour maps in the forward,
// upstream gradients in the backward): each job's NHWC copy is bf16 (one RNE rounding) or float32.
// 64 x 64 tiles again; loads take 4 pixels of one channel (16 bytes; one by one when HW % 4),
// the LDS image is [pixel][channel] f32 with rows of 65 words (the transposing writes and the
// row reads both land on 64 distinct banks), stores take 8 channels of one pixel: one 16-byte
// store in bf16, two in float32.
struct NhwcJobsF32 {
  const float* src[NHWC_MAXJOB];
  void* dst[NHWC_MAXJOB];
  int C[NHWC_MAXJOB], HW[NHWC_MAXJOB], tp[NHWC_MAXJOB], tc[NHWC_MAXJOB], f32[NHWC_MAXJOB];
  int block0[NHWC_MAXJOB + 1];  // first block of each job; block0[n] = grid
  int n;
};
__global__ __launch_bounds__(256) void k_nchw_to_nhwc_multi_f32(const NhwcJobsF32 J) {
  __shared__ float tile[64][65];
  int j = 0;
#pragma unroll
  for (int i = 1; i < NHWC_MAXJOB; ++i)
    if (i < J.n && (int)blockIdx.x >= J.block0[i]) j = i;
  const float* src = J.src[j];
  const int C = J.C[j], HW = J.HW[j], per = J.tp[j] * J.tc[j];
  const int idx = blockIdx.x - J.block0[j], b = idx / per, t = idx - b * per;
  const int p0 = (t % J.tp[j]) * 64, c0 = (t / J.tp[j]) * 64;
  const bool vec = (HW & 3) == 0;
  float4 q[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {  // all four loads in flight together
    const int v = threadIdx.x + 256 * k, cl = v >> 4, pl = (v & 15) * 4;  // channel, 4-pixel group
    const int c = c0 + cl, p = p0 + pl;
    const float* row = src + ((long long)b * C + c) * HW;
    q[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < C) {
      if (vec) {
        if (p < HW) q[k] = *reinterpret_cast<const float4*>(row + p);
      } else {
        if (p < HW) q[k].x = row[p];
        if (p + 1 < HW) q[k].y = row[p + 1];
        if (p + 2 < HW) q[k].z = row[p + 2];
        if (p + 3 < HW) q[k].w = row[p + 3];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int v = threadIdx.x + 256 * k, cl = v >> 4, pl = (v & 15) * 4;
    tile[pl][cl] = q[k].x;
    tile[pl + 1][cl] = q[k].y;
    tile[pl + 2][cl] = q[k].z;
    tile[pl + 3][cl] = q[k].w;
  }
  __syncthreads();
  const bool f32 = J.f32[j] != 0;  // workgroup-uniform
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int v = threadIdx.x + 256 * k, pl = v >> 3, cl = (v & 7) * 8;  // pixel, 8-channel group
    const int p = p0 + pl, c = c0 + cl;
    if (p >= HW || c >= C) continue;
    float e[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) e[i] = tile[pl][cl + i];
    const long long o = ((long long)b * HW + p) * C + c;
    if (f32) {
      float* d = (float*)J.dst[j] + o;
      *reinterpret_cast<float4*>(d) = make_float4(e[0], e[1], e[2], e[3]);
      *reinterpret_cast<float4*>(d + 4) = make_float4(e[4], e[5], e[6], e[7]);
    } else {
      *reinterpret_cast<uint4*>((bf16_t*)J.dst[j] + o) =
          make_uint4(pack_bf16x2(e[0], e[1]), pack_bf16x2(e[2], e[3]), pack_bf16x2(e[4], e[5]), pack_bf16x2(e[6], e[7]));
    }
  }
}

// Fills what NhwcJobs and NhwcJobsF32 share from the n host jobs: pointers, shapes, 64 x 64 tile
// counts and each job's first block; the slots past n stay zero.  check(job) holds the form's own
// requirements and runs right after the job's argument check.  -> the grid in J.block0[n].
template <typename Jobs, typename Job, typename Check>
int nhwc_job_table(int n, const Job* jobs, Jobs& J, Check&& check) {
  RGBD_REQUIRE(n >= 1 && n <= NHWC_MAXJOB && jobs, RGBD_E_ARG);
  J = Jobs{};
  long long blocks = 0;
  for (int i = 0; i < n; ++i) {
    const Job& q = jobs[i];
    RGBD_REQUIRE(q.src && q.dst && q.B > 0 && q.C > 0 && q.H > 0 && q.W > 0, RGBD_E_ARG);
    if (const int rc = check(q)) return rc;
    RGBD_REQUIRE((long long)q.H * q.W < (1ll << 31), RGBD_E_SHAPE);
    J.src[i] = static_cast<std::remove_reference_t<decltype(J.src[i])>>(q.src);
    J.dst[i] = static_cast<std::remove_reference_t<decltype(J.dst[i])>>(q.dst);
    J.C[i] = q.C;
    J.HW[i] = q.H * q.W;
    J.tp[i] = ceil_div((long long)q.H * q.W, 64);
    J.tc[i] = ceil_div(q.C, 64);
    J.block0[i] = (int)blocks;
    blocks += (long long)q.B * J.tp[i] * J.tc[i];
  }
  RGBD_REQUIRE(blocks < (1ll << 31), RGBD_E_SHAPE);
  for (int i = n; i <= NHWC_MAXJOB; ++i) J.block0[i] = (int)blocks;
  J.n = n;
  return RGBD_OK;
}

}  // namespace

extern "C" {

const char* rgbd_version(void) { return "rgbd_hip 0.1.0 (gfx950)"; }

int rgbd_nchw_to_nhwc(int dtype, const void* src, void* dst, int B, int C, int H, int W, void* stream) {
  RGBD_REQUIRE(src && dst && B > 0 && C > 0 && H > 0 && W > 0, RGBD_E_ARG);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == RGBD_BF16 && ((long long)H * W) % 8 == 0 && C % 8 == 0) {
    k_nchw_to_nhwc_v8<<<dim3(ceil_div((long long)H * W, 64), ceil_div(C, 64), B), 256, 0, s>>>(
        (const bf16_t*)src, (bf16_t*)dst, C, H * W);
    RGBD_CHECK_LAUNCH();
    return RGBD_OK;
  }
  dim3 grid(ceil_div((long long)H * W, 32), ceil_div(C, 32), B);
  if (dtype == RGBD_F32)
    k_nchw_to_nhwc<float><<<grid, 256, 0, s>>>((const float*)src, (float*)dst, C, H * W);
  else if (dtype == RGBD_BF16)
    k_nchw_to_nhwc<bf16_t><<<grid, 256, 0, s>>>((const bf16_t*)src, (bf16_t*)dst, C, H * W);
  else
    return RGBD_E_DTYPE;
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

int rgbd_nchw_to_nhwc_multi(int n, const rgbd_nhwc_job* jobs, void* stream) {
  NhwcJobs J;
  const int rc = nhwc_job_table(n, jobs, J, [](const rgbd_nhwc_job& q) -> int {
    RGBD_REQUIRE(q.C % 8 == 0, RGBD_E_SHAPE);  // 16-byte NHWC stores
    return RGBD_OK;
  });
  if (rc) return rc;
  k_nchw_to_nhwc_multi<<<(unsigned)J.block0[n], 256, 0, (hipStream_t)stream>>>(J);
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

int rgbd_nchw_to_nhwc_multi_f32(int n, const rgbd_nhwc_job_f32* jobs, void* stream) {
  NhwcJobsF32 J;
  const int rc = nhwc_job_table(n, jobs, J, [](const rgbd_nhwc_job_f32& q) -> int {
    RGBD_REQUIRE(q.dst_dtype == RGBD_F32 || q.dst_dtype == RGBD_BF16, RGBD_E_DTYPE);
    RGBD_REQUIRE(q.C % 8 == 0, RGBD_E_SHAPE);  // 16-byte NHWC stores
    RGBD_REQUIRE(((uintptr_t)q.src & 15) == 0 && ((uintptr_t)q.dst & 15) == 0, RGBD_E_ARG);  // 16-byte accesses
    return RGBD_OK;
  });
  if (rc) return rc;
  for (int i = 0; i < n; ++i) J.f32[i] = jobs[i].dst_dtype == RGBD_F32;
  k_nchw_to_nhwc_multi_f32<<<(unsigned)J.block0[n], 256, 0, (hipStream_t)stream>>>(J);
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

}  // extern "C"
