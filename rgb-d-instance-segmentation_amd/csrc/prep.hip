// K1 (DGGM-pre + 10-channel assembly) for gfx950.
//
// K1 follows calculate_gradient_features (reference mask2former/utils/data_process.py:1247-1305)
// as called by map_10channel_case2 (mask2former/utils/dataloader.py:386-425).  The Sobel sums
// of u8 depth are exact integers; sqrt and the normalising division use IEEE-rounded
// intrinsics, so the planes are bit-exact to the numpy/OpenCV float32 result.
//
// Two launches: pass 1 writes planes 0..5, the mask (plane 9) and the raw gradient magnitude
// (plane 6, scratch) and one (min over mag > 0, max) partial per block; pass 2 reduces its image's
// partials and normalises the magnitude into planes 6..8.  Each pass has a quad form (W % 4 == 0,
// 16-byte accesses) and a scalar form (any W) that share the partials and their reduction.
#include <cstdlib>

#include "common.hpp"
#include "timing.hpp"

using namespace rgbd;

namespace {

// image_mean / image_std of the reference's processor config
// (mask2former/checkpoints/standard/preprocessor_config.json), rounded to float32 as
// transformers' normalize does (np.array(mean, dtype=image.dtype)).  The config's std[1],
// 0.2239999920129776, is one float32 ulp below 0.224f.
__constant__ float kMean[3] = {0.48500001430511475f, 0.4560000002384186f, 0.4059999883174896f};
__constant__ float kStd[3] = {0.2290000021457672f, 0.2239999920129776f, 0.22499999403953552f};
constexpr double kRescale = 0.00392156862745098;  // rescale_factor of the same config

__device__ __forceinline__ int reflect101(int i, int n) {
  if (n == 1) return 0;
  if (i < 0) return -i;
  if (i >= n) return 2 * n - 2 - i;
  return i;
}

__device__ __forceinline__ float norm_u8(uint8_t v, int c) {
  // Mask2FormerImageProcessor (dataloader.py:405-410): transformers image_transforms.rescale
  // multiplies in float64 and rounds once to float32; normalize is (x - mean_c) / std_c in
  // float32, one rounding per op.
  const float x = (float)__dmul_rn((double)v, kRescale);
  return div_rn(__fsub_rn(x, kMean[c]), kStd[c]);
}

// The end of both pass-1 kernels: the block's (min over mag > 0, max) partial, reduced by pass 2
// (no same-address atomics: 256 blocks of one image serialising on one L2 line cost ~25 us).
// min/max are exact in any order, so the planes do not depend on the grid.
__device__ __forceinline__ void store_block_partial(float vmin, float vmax, int b, float2* __restrict__ part) {
  vmax = -wave_min(-vmax);
  vmin = wave_min(vmin);
  __shared__ float rmax[4], rmin[4];
  if ((threadIdx.x & 63) == 0) {
    rmax[threadIdx.x >> 6] = vmax;
    rmin[threadIdx.x >> 6] = vmin;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    part[(long long)b * gridDim.x + blockIdx.x] =
        make_float2(fminf(fminf(rmin[0], rmin[1]), fminf(rmin[2], rmin[3])),
                    fmaxf(fmaxf(rmax[0], rmax[1]), fmaxf(rmax[2], rmax[3])));
}

// Scalar pass 1 (W % 4 != 0 or unaligned buffers): one pixel per thread and iteration.
__global__ __launch_bounds__(256) void k_prep_pass1(const uint8_t* __restrict__ rgb,
                                                    const uint8_t* __restrict__ depth, int H, int W,
                                                    float* __restrict__ pv, float2* __restrict__ part) {
  const int b = blockIdx.y;
  const long long HW = (long long)H * W;
  const uint8_t* d = depth + b * HW;
  float* out = pv + b * 10 * HW;
  float vmax = 0.f, vmin = __uint_as_float(0x7f800000u);
  for (int p = blockIdx.x * 256 + threadIdx.x; p < (int)HW; p += 256 * gridDim.x) {
    const int y = p / W, x = p % W;
    const uint8_t dv = d[p];
    if (rgb) {
      const uint8_t* px = rgb + (b * HW + p) * 3;
      for (int c = 0; c < 3; ++c) out[c * HW + p] = norm_u8(px[c], c);
    }
    for (int c = 0; c < 3; ++c) out[(3 + c) * HW + p] = norm_u8(dv, c);
    const int ym = reflect101(y - 1, H), yp = reflect101(y + 1, H);
    const int xm = reflect101(x - 1, W), xp = reflect101(x + 1, W);
    auto at = [&](int yy, int xx) { return (int)d[(long long)yy * W + xx]; };
    const int gx = (at(ym, xp) - at(ym, xm)) + 2 * (at(y, xp) - at(y, xm)) + (at(yp, xp) - at(yp, xm));
    const int gy = (at(yp, xm) - at(ym, xm)) + 2 * (at(yp, x) - at(ym, x)) + (at(yp, xp) - at(ym, xp));
    float mag = sqrt_rn((float)(gx * gx + gy * gy));  // exact integer argument (< 2^24)
    if (dv == 0) mag = 0.f;                               // invalid depth (:1265, :1278)
    out[6 * HW + p] = mag;                                // scratch until pass 2
    out[9 * HW + p] = mag > 0.f ? 1.f : 0.f;              // valid-gradient mask (:1282)
    vmax = fmaxf(vmax, mag);
    if (mag > 0.f) vmin = fminf(vmin, mag);
  }
  store_block_partial(vmin, vmax, b, part);
}

// Quad pass 1 (W % 4 == 0, every NYUv2 / RealSense width): a thread owns 4 x-consecutive
// pixels — one 4-byte depth load per stencil row plus the two reflected edge bytes, three 4-byte
// RGB loads, and one 16-byte store per output plane — instead of 9 byte loads and 8 scalar
// stores per pixel.  Same arithmetic, same order per pixel, so the planes stay bit-exact.
__device__ __forceinline__ void row6(const uint8_t* __restrict__ row, int x0, int W, int (&v)[6]) {
  const uint32_t c = *reinterpret_cast<const uint32_t*>(row + x0);
  v[0] = row[reflect101(x0 - 1, W)];
  v[1] = c & 0xff;
  v[2] = (c >> 8) & 0xff;
  v[3] = (c >> 16) & 0xff;
  v[4] = c >> 24;
  v[5] = row[reflect101(x0 + 4, W)];
}

__global__ __launch_bounds__(256) void k_prep_pass1_q(const uint8_t* __restrict__ rgb,
                                                      const uint8_t* __restrict__ depth, int H, int W,
                                                      float* __restrict__ pv, float2* __restrict__ part) {
  const int b = blockIdx.y;
  const long long HW = (long long)H * W;
  const int WQ = W >> 2;
  const uint8_t* d = depth + b * HW;
  float* out = pv + b * 10 * HW;
  float vmax = 0.f, vmin = __uint_as_float(0x7f800000u);
  const int nq = (int)(HW >> 2);
  for (int q = blockIdx.x * 256 + threadIdx.x; q < nq; q += 256 * gridDim.x) {
    const int y = q / WQ, x0 = (q - y * WQ) * 4;
    const long long p = (long long)y * W + x0;
    int up[6], mid[6], dn[6];
    row6(d + (long long)reflect101(y - 1, H) * W, x0, W, up);
    row6(d + (long long)y * W, x0, W, mid);
    row6(d + (long long)reflect101(y + 1, H) * W, x0, W, dn);
    if (rgb) {
      const uint32_t* px = reinterpret_cast<const uint32_t*>(rgb + (b * HW + p) * 3);
      const uint32_t w0 = px[0], w1 = px[1], w2 = px[2];
      const uint8_t c[12] = {(uint8_t)w0, (uint8_t)(w0 >> 8), (uint8_t)(w0 >> 16), (uint8_t)(w0 >> 24),
                             (uint8_t)w1, (uint8_t)(w1 >> 8), (uint8_t)(w1 >> 16), (uint8_t)(w1 >> 24),
                             (uint8_t)w2, (uint8_t)(w2 >> 8), (uint8_t)(w2 >> 16), (uint8_t)(w2 >> 24)};
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
        *reinterpret_cast<float4*>(out + ch * HW + p) =
            make_float4(norm_u8(c[ch], ch), norm_u8(c[3 + ch], ch), norm_u8(c[6 + ch], ch), norm_u8(c[9 + ch], ch));
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
      *reinterpret_cast<float4*>(out + (3 + ch) * HW + p) =
          make_float4(norm_u8(mid[1], ch), norm_u8(mid[2], ch), norm_u8(mid[3], ch), norm_u8(mid[4], ch));
    float mag[4], msk[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int l = i, c = i + 1, r = i + 2;
      const int gx = (up[r] - up[l]) + 2 * (mid[r] - mid[l]) + (dn[r] - dn[l]);
      const int gy = (dn[l] - up[l]) + 2 * (dn[c] - up[c]) + (dn[r] - up[r]);
      float m = sqrt_rn((float)(gx * gx + gy * gy));  // exact integer argument (< 2^24)
      if (mid[c] == 0) m = 0.f;                         // invalid depth (:1265, :1278)
      mag[i] = m;
      msk[i] = m > 0.f ? 1.f : 0.f;                     // valid-gradient mask (:1282)
      vmax = fmaxf(vmax, m);
      if (m > 0.f) vmin = fminf(vmin, m);
    }
    *reinterpret_cast<float4*>(out + 6 * HW + p) = make_float4(mag[0], mag[1], mag[2], mag[3]);  // scratch
    *reinterpret_cast<float4*>(out + 9 * HW + p) = make_float4(msk[0], msk[1], msk[2], msk[3]);
  }
  store_block_partial(vmin, vmax, b, part);
}

// Pass 2: every block reduces its image's nparts partials, then normalises VW pixels per thread
// and iteration (VW = 4: 16-byte accesses, HW % 4 == 0; VW = 1: any HW).
template <int VW>
__global__ __launch_bounds__(256) void k_prep_pass2(int H, int W, float* __restrict__ pv,
                                                    const float2* __restrict__ part, int nparts) {
  const int b = blockIdx.y;
  const long long HW = (long long)H * W;
  float* out = pv + b * 10 * HW;
  float lmn = __uint_as_float(0x7f800000u), lmx = 0.f;
  for (int i = threadIdx.x; i < nparts; i += 256) {
    const float2 v = part[(long long)b * nparts + i];
    lmn = fminf(lmn, v.x);
    lmx = fmaxf(lmx, v.y);
  }
  lmn = wave_min(lmn);
  lmx = -wave_min(-lmx);
  __shared__ float smn[4], smx[4];
  if ((threadIdx.x & 63) == 0) {
    smn[threadIdx.x >> 6] = lmn;
    smx[threadIdx.x >> 6] = lmx;
  }
  __syncthreads();
  const float mn = fminf(fminf(smn[0], smn[1]), fminf(smn[2], smn[3]));
  const float mx = fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3]));
  const uint32_t mnb = __float_as_uint(mn);
  const bool scale = (mnb != 0x7f800000u) && (mx > mn);  // :1285-1293
  const float den = __fsub_rn(mx, mn);
  for (long long p = (blockIdx.x * 256ll + threadIdx.x) * VW; p < HW; p += 256ll * VW * gridDim.x) {
    if constexpr (VW == 4) {
      const float4 m = *reinterpret_cast<const float4*>(out + 6 * HW + p);
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (scale)
        v = make_float4(div_rn(__fsub_rn(m.x, mn), den), div_rn(__fsub_rn(m.y, mn), den),
                        div_rn(__fsub_rn(m.z, mn), den), div_rn(__fsub_rn(m.w, mn), den));
      *reinterpret_cast<float4*>(out + 6 * HW + p) = v;
      *reinterpret_cast<float4*>(out + 7 * HW + p) = v;
      *reinterpret_cast<float4*>(out + 8 * HW + p) = v;
    } else {
      const float mag = out[6 * HW + p];
      const float v = scale ? div_rn(__fsub_rn(mag, mn), den) : 0.f;
      out[6 * HW + p] = v;
      out[7 * HW + p] = v;
      out[8 * HW + p] = v;
    }
  }
}

constexpr int kPrepMaxParts = 1024;  // pass-1 blocks per image, at most
// The partials follow a 256-byte-aligned header of 8 bytes per image that earlier versions kept
// their min/max records in; the size and the partials' place are what callers have always got.
size_t prep_parts_offset(int B) { return align256(8 * (size_t)B); }

}  // namespace

extern "C" {

size_t rgbd_assemble_workspace_size(int B) {
  const int nb = B > 0 ? B : 1;
  return prep_parts_offset(nb) + align256(sizeof(float2) * kPrepMaxParts * (size_t)nb);
}

int rgbd_assemble_pixel_values(const uint8_t* rgb_u8, const uint8_t* depth_u8, int B, int H, int W,
                               float* pv, void* ws, void* stream) {
  RGBD_REQUIRE(depth_u8 && pv && ws, RGBD_E_ARG);
  RGBD_REQUIRE(B > 0 && H > 0 && W > 0, RGBD_E_ARG);
  hipStream_t s = (hipStream_t)stream;
  TimerScope ts("assemble", s);
  const long long HW = (long long)H * W;
  RGBD_REQUIRE(HW < (1ll << 31), RGBD_E_SHAPE);
  float2* part = (float2*)((char*)ws + prep_parts_offset(B));
  if (W % 4 == 0 && ((uintptr_t)pv & 15) == 0 && ((uintptr_t)depth_u8 & 3) == 0 && ((uintptr_t)rgb_u8 & 3) == 0) {
    const int nparts = (int)std::min<long long>(std::min<long long>(ceil_div(HW / 4, 256), std::max(2048 / B, 16)),
                                                kPrepMaxParts);
    dim3 grid((unsigned)nparts, B);
    k_prep_pass1_q<<<grid, 256, 0, s>>>(rgb_u8, depth_u8, H, W, pv, part);
    k_prep_pass2<4><<<grid, 256, 0, s>>>(H, W, pv, part, nparts);
  } else {
    const int nparts = (int)std::min<long long>(ceil_div(HW, 256), 128);
    dim3 grid((unsigned)nparts, B);
    k_prep_pass1<<<grid, 256, 0, s>>>(rgb_u8, depth_u8, H, W, pv, part);
    k_prep_pass2<1><<<grid, 256, 0, s>>>(H, W, pv, part, nparts);
  }
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

}  // extern "C"
