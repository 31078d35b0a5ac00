// Colour-map gradients of the fused hot path's end-to-end mode (rgbd_color_grads): up to four jobs
//   out = G + D   (NCHW, in G's dtype; D absent: out = G + G)
// in one launch, where D is the cascade gradient d cp1 as the DSAM dX legs leave it: NCHW (the
// float32 mode) or NHWC (the bf16 modes).  The inverse of k_nchw_to_nhwc_multi (layout.hip)
// with an add on the way out: an NHWC source goes through a padded LDS tile, everything else is a
// flat elementwise pass.  Each element is one float32 add and one rounding to G's dtype.
// HBM-bound: reads G and D once, writes out once; no atomics, no workspace.
#include "common.hpp"
#include "timing.hpp"

namespace rgbd {
namespace {

constexpr int CG_MAXJOB = 4;
constexpr int CG_TILE = 64;              // NHWC jobs: 64 pixels x 64 channels per workgroup
constexpr int CG_FLAT = 256 * 8 * 2;     // flat jobs: elements per workgroup
enum : int { CG_G_BF16 = 1, CG_D_BF16 = 2, CG_D_NHWC = 4, CG_VEC_G = 8, CG_VEC_D = 16 };

struct ColorGradJobs {
  const void* g[CG_MAXJOB];
  const void* d[CG_MAXJOB];
  void* out[CG_MAXJOB];
  long long total[CG_MAXJOB];  // B C H W
  int C[CG_MAXJOB], HW[CG_MAXJOB], tp[CG_MAXJOB], tc[CG_MAXJOB], flags[CG_MAXJOB];
  int block0[CG_MAXJOB + 1];  // first block of each job; block0[n] = grid
  int n;
};

// 8 consecutive elements from element offset off, widened to float32: one 16-byte (bf16) or two
// 16-byte (float32) loads when vec, else the first nv one by one (the rest are zero)
__device__ __forceinline__ void load8(const void* base, long long off, bool bf, bool vec, int nv, float v[8]) {
  if (bf) {
    const bf16_t* p = (const bf16_t*)base + off;
    if (vec) {
      const uint4 u = *reinterpret_cast<const uint4*>(p);
      const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[2 * e] = __uint_as_float(w[e] << 16);
        v[2 * e + 1] = __uint_as_float(w[e] & 0xffff0000u);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = e < nv ? bf16_to_f32(p[e]) : 0.f;
    }
  } else {
    const float* p = (const float*)base + off;
    if (vec) {
      const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
      v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
      v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = e < nv ? p[e] : 0.f;
    }
  }
}

// the store of load8's shape; bf16 rounds to nearest even with the same instruction on both paths
__device__ __forceinline__ void store8(void* base, long long off, bool bf, bool vec, int nv, const float v[8]) {
  if (bf) {
    bf16_t* p = (bf16_t*)base + off;
    const uint4 u = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]),
                               pack_bf16x2(v[6], v[7]));
    if (vec) {
      *reinterpret_cast<uint4*>(p) = u;
    } else {
      const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (e < nv) p[e] = (bf16_t)((e & 1) ? (w[e >> 1] >> 16) : (w[e >> 1] & 0xffffu));
    }
  } else {
    float* p = (float*)base + off;
    if (vec) {
      *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
      *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (e < nv) p[e] = v[e];
    }
  }
}

__global__ __launch_bounds__(256) void k_color_grads(const ColorGradJobs J) {
  // [channel][pixel] float32, rows of 65 words: the transposing writes (8 pixels x 8 channel
  // groups per wave) and the row reads (8 channels x 8 pixel groups) both land on 64 distinct banks
  __shared__ float tile[CG_TILE][CG_TILE + 1];
  int j = 0;
#pragma unroll
  for (int i = 1; i < CG_MAXJOB; ++i)
    if (i < J.n && (int)blockIdx.x >= J.block0[i]) j = i;
  const void* G = J.g[j];
  const void* D = J.d[j];
  void* out = J.out[j];
  const int fl = J.flags[j];
  const bool gbf = fl & CG_G_BF16, dbf = fl & CG_D_BF16, vg = fl & CG_VEC_G, vd = fl & CG_VEC_D;
  const int idx = blockIdx.x - J.block0[j];
  if (!(fl & CG_D_NHWC)) {  // flat: D absent or NCHW like G
    const long long total = J.total[j];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const long long e0 = (long long)idx * CG_FLAT + (threadIdx.x + 256 * k) * 8;
      if (e0 >= total) continue;
      const int nv = total - e0 < 8 ? (int)(total - e0) : 8;
      const bool full = nv == 8;
      float g[8], d[8], o[8];
      load8(G, e0, gbf, vg && full, nv, g);
      if (D) {
        load8(D, e0, dbf, vd && full, nv, d);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = g[e] + d[e];
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = g[e] + g[e];
      }
      store8(out, e0, gbf, vg && full, nv, o);
    }
    return;
  }
  const int C = J.C[j], HW = J.HW[j], per = J.tp[j] * J.tc[j];
  const int b = idx / per, t = idx - b * per;
  const int p0 = (t % J.tp[j]) * CG_TILE, c0 = (t / J.tp[j]) * CG_TILE;
  float d8[2][8];
#pragma unroll
  for (int k = 0; k < 2; ++k) {  // both loads in flight together
    const int v = threadIdx.x + 256 * k, pl = v >> 3, cl = (v & 7) * 8;  // pixel, 8-channel group
    const int p = p0 + pl, c = c0 + cl;
#pragma unroll
    for (int e = 0; e < 8; ++e) d8[k][e] = 0.f;
    if (p < HW && c < C) load8(D, ((long long)b * HW + p) * C + c, dbf, vd, 8, d8[k]);  // C % 8 == 0
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int v = threadIdx.x + 256 * k, pl = v >> 3, cl = (v & 7) * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) tile[cl + e][pl] = d8[k][e];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int v = threadIdx.x + 256 * k, cl = v >> 3, pl = (v & 7) * 8;  // channel, 8-pixel group
    const int c = c0 + cl, p = p0 + pl;
    if (c >= C || p >= HW) continue;
    const int nv = HW - p < 8 ? HW - p : 8;
    const bool vec = vg && nv == 8;  // CG_VEC_G of an NHWC job implies HW % 8 == 0
    const long long off = ((long long)b * C + c) * HW + p;
    float g[8], o[8];
    load8(G, off, gbf, vec, nv, g);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = g[e] + tile[cl][pl + e];
    store8(out, off, gbf, vec, nv, o);
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace
}  // namespace rgbd

using namespace rgbd;

extern "C" int rgbd_color_grads(int n, const rgbd_color_grad_job* jobs, void* stream) {
  RGBD_REQUIRE(n >= 1 && n <= CG_MAXJOB && jobs, RGBD_E_ARG);
  ColorGradJobs J = {};
  long long blocks = 0;
  int m = 0;  // jobs with work
  for (int i = 0; i < n; ++i) {
    const rgbd_color_grad_job& q = jobs[i];
    RGBD_REQUIRE(q.g && q.out && q.B >= 0 && q.C >= 0 && q.H >= 0 && q.W >= 0, RGBD_E_ARG);
    RGBD_REQUIRE(q.g_dtype == RGBD_F32 || q.g_dtype == RGBD_BF16, RGBD_E_DTYPE);
    RGBD_REQUIRE(!q.d || q.d_dtype == RGBD_F32 || q.d_dtype == RGBD_BF16, RGBD_E_DTYPE);
    const bool nhwc = q.d && q.d_nhwc;
    RGBD_REQUIRE(!nhwc || q.C % 8 == 0, RGBD_E_SHAPE);  // 8-channel items of the NHWC source
    const long long hw = (long long)q.H * q.W;
    RGBD_REQUIRE(hw < (1ll << 31) && (long long)q.B * q.C < (1ll << 31), RGBD_E_SHAPE);
    const long long total = hw * q.B * q.C;
    RGBD_REQUIRE(total < (1ll << 31), RGBD_E_SHAPE);
    if (total == 0) continue;
    J.g[m] = q.g; J.d[m] = q.d; J.out[m] = q.out;
    J.total[m] = total;
    J.C[m] = q.C;
    J.HW[m] = (int)hw;
    int fl = (q.g_dtype == RGBD_BF16 ? CG_G_BF16 : 0) | (q.d && q.d_dtype == RGBD_BF16 ? CG_D_BF16 : 0);
    // 16-byte accesses: aligned pointers and, where rows of H W pixels are walked, H W % 8 == 0
    if (aligned16(q.g) && aligned16(q.out) && (!nhwc || hw % 8 == 0)) fl |= CG_VEC_G;
    if (q.d && aligned16(q.d)) fl |= CG_VEC_D;
    J.block0[m] = (int)blocks;
    if (nhwc) {
      fl |= CG_D_NHWC;
      J.tp[m] = ceil_div(hw, CG_TILE);
      J.tc[m] = ceil_div(q.C, CG_TILE);
      blocks += (long long)q.B * J.tp[m] * J.tc[m];
    } else {
      blocks += (total + CG_FLAT - 1) / CG_FLAT;
    }
    J.flags[m] = fl;
    ++m;
  }
  RGBD_REQUIRE(blocks < (1ll << 31), RGBD_E_SHAPE);
  if (m == 0) return RGBD_OK;  // nothing to do
  for (int i = m; i <= CG_MAXJOB; ++i) J.block0[i] = (int)blocks;
  J.n = m;
  TimerScope ts("color_grads", (hipStream_t)stream);
  k_color_grads<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(J);
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}
