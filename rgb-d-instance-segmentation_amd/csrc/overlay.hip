// f5: painting a prediction over its frame on the device (gfx950).
//
// Reference: mask2former/predictor.py:295-330 (_create_gt_overlay_with_consistent_colors) and
// :1286-1320 (_create_prediction_overlay) — per segment of segments_info, for the pixels whose map
// value equals the segment id and for each channel,
//     overlay[mask, c] = (1 - alpha) * overlay[mask, c] + alpha * color[c]
// on a float32 copy of the image, then np.clip(overlay, 0, 255).astype(np.uint8).  Under NumPy 2
// promotion the Python-float weight and colour term take the array's float32, so per channel
//     v = float32(1 - alpha) * float32(x) + float32(alpha * c)      two roundings: product, sum
// and a segment id occurs once in segments_info, so every pixel is blended at most once.
//
//   k_overlay_lut      one thread per (image, id): the last top-k slot whose seg_id equals the id
//                      decides its colour (a scan of the Q slots, so the result does not depend on
//                      the order threads run in); ids no slot names stay -1.
//   k_overlay_blend16  the 16-byte path, when rgb, seg and out are all 16-byte aligned: one lane per
//                      16 consecutive pixels of the flat [B H W] range — three 16-byte RGB loads,
//                      four 16-byte map loads, three 16-byte stores.  The image a pixel belongs to
//                      (the table is per image) is tracked per pixel, so a group may straddle any
//                      number of images; the last, partial group goes pixel by pixel.
//   k_overlay_blend1   every other alignment: one thread per pixel, byte accesses (the map cell is
//                      assembled from bytes unless seg is 4-byte aligned).
//
// alpha * c is formed in float64 and rounded once, as Python does; the product and the sum are
// __fmul_rn / __fadd_rn, so nothing contracts them whatever the compile flags.
#include <cmath>

#include "common.hpp"
#include "label_cell.hpp"  // cell_id: the id a map cell names

using namespace rgbd;

namespace {

constexpr int OV_THR = 256;
constexpr int OV_GROUP = 16;  // pixels per lane on the 16-byte path

__global__ __launch_bounds__(OV_THR) void k_overlay_lut(const int* __restrict__ seg_id, const int* __restrict__ topk_idx,
                                                       int Q, int C, const uint8_t* __restrict__ palette, int n_colors,
                                                       int color_by, int32_t* __restrict__ lut, int n_ids) {
  const int b = blockIdx.y;
  const int id = blockIdx.x * OV_THR + threadIdx.x;
  if (id >= n_ids) return;
  const int* sid = seg_id + (long long)b * Q;
  int slot = -1;
  for (int j = 0; j < Q; ++j)
    if (sid[j] == id) slot = j;
  int32_t v = -1;
  if (slot >= 0) {
    int k = id;
    if (color_by == 0) {
      k = topk_idx[(long long)b * Q + slot] % C;
      if (k < 0) k += C;  // Python's %
    }
    const uint8_t* p = palette + 3 * (k % n_colors);
    v = (int32_t)p[0] | ((int32_t)p[1] << 8) | ((int32_t)p[2] << 16);
  }
  lut[(long long)b * n_ids + id] = v;
}

__device__ __forceinline__ uint32_t blend_channel(uint32_t x, uint32_t c, float w0, double alpha) {
  const float t = (float)(alpha * (double)c);
  float v = __fadd_rn(__fmul_rn(w0, (float)x), t);
  v = fminf(fmaxf(v, 0.f), 255.f);
  return (uint32_t)v;  // toward zero
}

template <bool F32>
__global__ __launch_bounds__(OV_THR) void k_overlay_blend16(const uint8_t* __restrict__ rgb, const uint32_t* __restrict__ seg,
                                                           const int32_t* __restrict__ lut, long long npix, long long hw,
                                                           int n_ids, float w0, double alpha, uint8_t* __restrict__ out) {
  const long long g = blockIdx.x * (long long)OV_THR + threadIdx.x;
  const long long p0 = g * OV_GROUP;
  if (p0 >= npix) return;
  long long b = p0 / hw;
  long long rem = p0 - b * hw;
  if (p0 + OV_GROUP <= npix) {
    const u32x4* src = reinterpret_cast<const u32x4*>(rgb + 3 * p0);
    const u32x4* sg = reinterpret_cast<const u32x4*>(seg + p0);
    const u32x4 r0 = src[0], r1 = src[1], r2 = src[2];
    const u32x4 s0 = sg[0], s1 = sg[1], s2 = sg[2], s3 = sg[3];
    uint32_t in[12] = {r0[0], r0[1], r0[2], r0[3], r1[0], r1[1], r1[2], r1[3], r2[0], r2[1], r2[2], r2[3]};
    const uint32_t cell[16] = {s0[0], s0[1], s0[2], s0[3], s1[0], s1[1], s1[2], s1[3],
                               s2[0], s2[1], s2[2], s2[3], s3[0], s3[1], s3[2], s3[3]};
    uint32_t o[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < OV_GROUP; ++k) {
      const int id = cell_id<F32>(cell[k], n_ids);
      const int32_t col = lut[b * n_ids + (id >= 0 ? id : 0)];
      const bool paint = id >= 0 && col >= 0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int byte = 3 * k + c;
        const uint32_t x = (in[byte >> 2] >> (8 * (byte & 3))) & 0xffu;
        const uint32_t y = blend_channel(x, ((uint32_t)col >> (8 * c)) & 0xffu, w0, alpha);
        o[byte >> 2] |= (paint ? y : x) << (8 * (byte & 3));
      }
      if (++rem == hw) {
        rem = 0;
        ++b;
      }
    }
    u32x4* dst = reinterpret_cast<u32x4*>(out + 3 * p0);
    dst[0] = u32x4{o[0], o[1], o[2], o[3]};
    dst[1] = u32x4{o[4], o[5], o[6], o[7]};
    dst[2] = u32x4{o[8], o[9], o[10], o[11]};
    return;
  }
  // the flat range's last, partial group
  for (long long p = p0; p < npix; ++p) {
    const int id = cell_id<F32>(seg[p], n_ids);
    const int32_t col = lut[b * n_ids + (id >= 0 ? id : 0)];
    const bool paint = id >= 0 && col >= 0;
    for (int c = 0; c < 3; ++c) {
      const uint32_t x = rgb[3 * p + c];
      const uint32_t y = blend_channel(x, ((uint32_t)col >> (8 * c)) & 0xffu, w0, alpha);
      out[3 * p + c] = (uint8_t)(paint ? y : x);
    }
    if (++rem == hw) {
      rem = 0;
      ++b;
    }
  }
}

template <bool F32>
__global__ __launch_bounds__(OV_THR) void k_overlay_blend1(const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ seg,
                                                          int seg_al4, const int32_t* __restrict__ lut, long long npix,
                                                          long long hw, int n_ids, float w0, double alpha,
                                                          uint8_t* __restrict__ out) {
  const long long p = blockIdx.x * (long long)OV_THR + threadIdx.x;
  if (p >= npix) return;
  const long long b = p / hw;
  uint32_t bits;
  if (seg_al4) {
    bits = reinterpret_cast<const uint32_t*>(seg)[p];
  } else {
    const uint8_t* q = seg + 4 * p;
    bits = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
  }
  const int id = cell_id<F32>(bits, n_ids);
  const int32_t col = lut[b * n_ids + (id >= 0 ? id : 0)];
  const bool paint = id >= 0 && col >= 0;
  for (int c = 0; c < 3; ++c) {
    const uint32_t x = rgb[3 * p + c];
    const uint32_t y = blend_channel(x, ((uint32_t)col >> (8 * c)) & 0xffu, w0, alpha);
    out[3 * p + c] = (uint8_t)(paint ? y : x);
  }
}

constexpr long long OV_MAX_PIX = 1ll << 36;  // keeps every grid below 2^31 blocks

}  // namespace

extern "C" {

int rgbd_overlay_lut(const int* seg_id, const int* topk_idx, int B, int Q, int C, const uint8_t* palette, int n_colors,
                     int color_by, int32_t* lut, int n_ids, void* stream) {
  RGBD_REQUIRE(seg_id && topk_idx && palette && lut, RGBD_E_ARG);
  RGBD_REQUIRE(B > 0 && Q > 0 && C > 0 && n_colors > 0 && n_ids > 0, RGBD_E_ARG);
  RGBD_REQUIRE(color_by == 0 || color_by == 1, RGBD_E_ARG);
  RGBD_REQUIRE(B <= 65535 && (long long)B * n_ids < (1ll << 31), RGBD_E_SHAPE);
  k_overlay_lut<<<dim3(ceil_div(n_ids, OV_THR), B), OV_THR, 0, (hipStream_t)stream>>>(seg_id, topk_idx, Q, C, palette,
                                                                                    n_colors, color_by, lut, n_ids);
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

int rgbd_overlay_blend(const uint8_t* rgb, const void* seg, int seg_dtype, const int32_t* lut, int B, int H, int W,
                       int n_ids, double alpha, uint8_t* out, void* stream) {
  RGBD_REQUIRE(rgb && seg && lut && out, RGBD_E_ARG);
  RGBD_REQUIRE(B > 0 && H > 0 && W > 0 && n_ids > 0, RGBD_E_ARG);
  RGBD_REQUIRE(std::isfinite(alpha), RGBD_E_ARG);
  RGBD_REQUIRE(seg_dtype == RGBD_F32 || seg_dtype == RGBD_I32, RGBD_E_DTYPE);
  const long long hw = (long long)H * W;
  RGBD_REQUIRE(hw <= OV_MAX_PIX / B && (long long)B * n_ids < (1ll << 31), RGBD_E_SHAPE);
  const long long npix = hw * B;
  // out is written while rgb is still being read by other lanes: the two may not overlap
  const uintptr_t r = (uintptr_t)rgb, o = (uintptr_t)out, nb = (uintptr_t)(3 * npix);
  RGBD_REQUIRE(r + nb <= o || o + nb <= r, RGBD_E_ARG);
  RGBD_REQUIRE(((uintptr_t)lut & 3) == 0, RGBD_E_ARG);
  const float w0 = (float)(1.0 - alpha);
  hipStream_t s = (hipStream_t)stream;
  const bool f32 = seg_dtype == RGBD_F32;
  if (((r | o | (uintptr_t)seg) & 15) == 0) {
    const unsigned grid = (unsigned)((npix + (long long)OV_GROUP * OV_THR - 1) / ((long long)OV_GROUP * OV_THR));
    auto* kern = f32 ? k_overlay_blend16<true> : k_overlay_blend16<false>;
    kern<<<grid, OV_THR, 0, s>>>(rgb, (const uint32_t*)seg, lut, npix, hw, n_ids, w0, alpha, out);
  } else {
    const unsigned grid = (unsigned)((npix + OV_THR - 1) / OV_THR);
    auto* kern = f32 ? k_overlay_blend1<true> : k_overlay_blend1<false>;
    kern<<<grid, OV_THR, 0, s>>>(rgb, (const uint8_t*)seg, ((uintptr_t)seg & 3) == 0, lut, npix, hw, n_ids, w0, alpha,
                                 out);
  }
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

}  // extern "C"
