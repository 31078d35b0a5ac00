// K2 (DGGM gated fusion fwd/bwd) for gfx950.
//
// K2 follows DepthGradientInjectionResidual.forward (custom_model.py:1204-1269) fused with the
// final sum backbone_k = cp1_k + cp2_k (custom_model.py:355).  A workgroup computes the
// resampled gate (3 bilinear taps x 4 + 1 nearest) of a pixel tile once into LDS and streams 32
// channel planes of that tile with vector accesses (8 pixels per lane where h*w allows).
//
// One kernel per direction (plus the backward's final reduction) serves up to four scales per
// launch; the single-scale entry points launch it with one scale.
#include <type_traits>

#include "common.hpp"
#include "timing.hpp"

using namespace rgbd;

namespace {

struct Gate {
  float g[3];
};

// torch upsample_bilinear2d (align_corners=False) source index + nearest (legacy floor).
__device__ __forceinline__ void src_lin(int dst, int in, int out, int& i0, int& i1, float& l1) {
  const float scale = (float)in / (float)out;
  float s = scale * (dst + 0.5f) - 0.5f;
  if (s < 0.f) s = 0.f;
  i0 = (int)s;
  i1 = i0 + ((i0 < in - 1) ? 1 : 0);
  l1 = s - (float)i0;
}
__device__ __forceinline__ int src_nearest(int dst, int in, int out) {
  const float scale = (float)in / (float)out;
  int s = (int)floorf((float)dst * scale);
  return s < in - 1 ? s : in - 1;
}

__device__ __forceinline__ Gate gate_at(const float* __restrict__ grad, const float* __restrict__ mask,
                                        int H, int W, int h, int w, int y, int x) {
  int y0, y1, x0, x1;
  float ly1, lx1;
  src_lin(y, H, h, y0, y1, ly1);
  src_lin(x, W, w, x0, x1, lx1);
  const float ly0 = 1.f - ly1, lx0 = 1.f - lx1;
  const long long HW = (long long)H * W;
  const float m = mask[(long long)src_nearest(y, H, h) * W + src_nearest(x, W, w)];
  Gate gt;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* gp = grad + c * HW;
    const float v = ly0 * (lx0 * gp[(long long)y0 * W + x0] + lx1 * gp[(long long)y0 * W + x1]) +
                    ly1 * (lx0 * gp[(long long)y1 * W + x0] + lx1 * gp[(long long)y1 * W + x1]);
    gt.g[c] = v * m;  // gated_depth_grad = bilinear * nearest(mask) (:1246)
  }
  return gt;
}

// Block = a tile of 64*PX pixels of one image x 32 channels; the tile's gates are computed once
// into LDS, each wave then owns 8 channels and each lane PX consecutive pixels: one 16-B (PX=8),
// 8-B (PX=4) or 2-B (PX=1) access per bf16 channel plane, PX the largest of 8/4/1 dividing h*w
// (so a lane's pixels are all valid or all past the end).  All 8 channels' loads are issued
// before any arithmetic.
constexpr int kBlkCh = 32;
constexpr int kWaveCh = 8;
constexpr int kRedStride = 36;  // floats per lane row of the bwd wave reduction

template <typename T, int PX> struct PxN;
template <int PX> struct PxN<float, PX> {
  static __device__ __forceinline__ void load(const float* p, float (&v)[PX]) {
    if constexpr (PX == 1) {
      v[0] = *p;
    } else {
#pragma unroll
      for (int q = 0; q < PX / 4; ++q) {
        const float4 a = ((const float4*)p)[q];
        v[4 * q] = a.x; v[4 * q + 1] = a.y; v[4 * q + 2] = a.z; v[4 * q + 3] = a.w;
      }
    }
  }
  static __device__ __forceinline__ void store(float* p, const float (&v)[PX]) {
    if constexpr (PX == 1) {
      *p = v[0];
    } else {
#pragma unroll
      for (int q = 0; q < PX / 4; ++q) ((float4*)p)[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
    }
  }
};
template <int PX> struct PxN<bf16_t, PX> {
  static __device__ __forceinline__ void load(const bf16_t* p, float (&v)[PX]) {
    if constexpr (PX == 1) {
      v[0] = bf16_to_f32(*p);
    } else {
      uint32_t w[PX / 2];
      if constexpr (PX == 8) {
        const uint4 u = *(const uint4*)p;
        w[0] = u.x; w[1] = u.y; w[2] = u.z; w[3] = u.w;
      } else {
        const uint2 u = *(const uint2*)p;
        w[0] = u.x; w[1] = u.y;
      }
#pragma unroll
      for (int j = 0; j < PX / 2; ++j) {
        v[2 * j] = __uint_as_float(w[j] << 16);
        v[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
      }
    }
  }
  static __device__ __forceinline__ void store(bf16_t* p, const float (&v)[PX]) {
    if constexpr (PX == 1) {
      *p = f32_to_bf16(v[0]);
    } else {
      uint32_t w[PX / 2];
#pragma unroll
      for (int j = 0; j < PX / 2; ++j) w[j] = (uint32_t)f32_to_bf16(v[2 * j]) | ((uint32_t)f32_to_bf16(v[2 * j + 1]) << 16);
      if constexpr (PX == 8)
        *(uint4*)p = make_uint4(w[0], w[1], w[2], w[3]);
      else
        *(uint2*)p = make_uint2(w[0], w[1]);
    }
  }
};


template <int PX>
struct TileGates {
  float g[3][PX];
  int p;       // first pixel of this lane within the image
  bool valid;  // the lane's PX pixels are inside the image
};

// Stage the tile's gates in LDS and return this lane's PX of them.
// Also stages the block's 32 channels of (w0, w1, w2, bias) into swb (clamped past C).
template <int PX>
__device__ __forceinline__ TileGates<PX> stage_gates(float (*sg)[512], float4* swb, const float* __restrict__ grad,
                                                     const float* __restrict__ mask, int H, int W, int h,
                                                     int w, int p0, const float* __restrict__ wt,
                                                     const float* __restrict__ bias, int C, int by) {
  constexpr int TP = 64 * PX;
  const int hw = h * w;
  if (threadIdx.x < kBlkCh) {
    const int c = min(by * kBlkCh + (int)threadIdx.x, C - 1);
    swb[threadIdx.x] = make_float4(wt[c * 3 + 0], wt[c * 3 + 1], wt[c * 3 + 2], bias[c]);
  }
#pragma unroll
  for (int i0 = 0; i0 < TP; i0 += 256) {
    const int i = i0 + threadIdx.x;
    const int p = p0 + i;
    if (i < TP) {
      Gate gt = {{0.f, 0.f, 0.f}};
      if (p < hw) gt = gate_at(grad, mask, H, W, h, w, p / w, p % w);
      sg[0][i] = gt.g[0];
      sg[1][i] = gt.g[1];
      sg[2][i] = gt.g[2];
    }
  }
  __syncthreads();
  TileGates<PX> t;
  const int lane = threadIdx.x & 63;
  t.p = p0 + PX * lane;
  t.valid = t.p < hw;
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int j = 0; j < PX; ++j) t.g[c][j] = sg[c][PX * lane + j];
  return t;
}

// One pixel's 8 channels [c0, c0+8) of an NHWC map -> v[cc][j] (cc < 8); C % 8 == 0.
template <typename T, int PX>
__device__ __forceinline__ void load_nhwc8(const T* p, float (&v)[kWaveCh][PX], int j) {
  if constexpr (sizeof(T) == 2) {
    const uint4 u = *reinterpret_cast<const uint4*>(p);
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      v[2 * q][j] = __uint_as_float(w[q] << 16);
      v[2 * q + 1][j] = __uint_as_float(w[q] & 0xffff0000u);
    }
  } else {
    const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
    v[0][j] = a.x; v[1][j] = a.y; v[2][j] = a.z; v[3][j] = a.w;
    v[4][j] = b.x; v[5][j] = b.y; v[6][j] = b.z; v[7][j] = b.w;
  }
}

// One (pixel tile bx, 32-channel block by) of the fused forward; the kernel below maps its flat
// block index onto it.
template <typename T, int PX, bool HAS1, bool CP1_NHWC = false>
__device__ __forceinline__ void dggm_fwd_block(float (*sg)[512], float4* swb, int bx, int by,
                                               const T* __restrict__ cp1, const T* __restrict__ color,
                                               const float* __restrict__ grad, const float* __restrict__ mask,
                                               long long pvs, int H, int W, int C, int h, int w,
                                               const float* __restrict__ wt, const float* __restrict__ bias,
                                               T* __restrict__ out) {
  constexpr int TP = 64 * PX;
  const int hw = h * w, tpi = (hw + TP - 1) / TP;
  const int b = bx / tpi, p0 = (bx % tpi) * TP;
  const TileGates<PX> t = stage_gates<PX>(sg, swb, grad + b * pvs, mask + b * pvs, H, W, h, w, p0, wt, bias, C, by);
  const int cw = by * kBlkCh + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * kWaveCh;
  if (!t.valid || cw >= C) return;
  float col[kWaveCh][PX], y[kWaveCh][PX];
#pragma unroll
  for (int cc = 0; cc < kWaveCh; ++cc) {
    const long long o = ((long long)b * C + min(cw + cc, C - 1)) * hw + t.p;
    PxN<T, PX>::load(color + o, col[cc]);
    if constexpr (HAS1 && !CP1_NHWC) PxN<T, PX>::load(cp1 + o, y[cc]);
  }
  if constexpr (HAS1 && CP1_NHWC)  // cp1 NHWC (the DSAM cascade's layout): 8 channels per pixel load
#pragma unroll
    for (int j = 0; j < PX; ++j) load_nhwc8<T, PX>(cp1 + ((long long)b * hw + t.p + j) * C + cw, y, j);
  __builtin_amdgcn_sched_barrier(0);  // keep the whole load batch ahead of the first use
#pragma unroll
  for (int cc = 0; cc < kWaveCh; ++cc) {
    const int c = min(cw + cc, C - 1);
    const float4 wb = swb[c - by * kBlkCh];
    const float w0 = wb.x, w1 = wb.y, w2 = wb.z, bc = wb.w;
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      const float pre = bc + w0 * t.g[0][j] + w1 * t.g[1][j] + w2 * t.g[2][j];
      const float cp2 = col[cc][j] + (pre > 0.f ? pre : 0.f);  // color_feat + depth_enhancement (:1255)
      y[cc][j] = HAS1 ? y[cc][j] + cp2 : cp2;
    }
  }
  // stores after all arithmetic: a per-channel guard between loads and uses would let the
  // compiler sink each load into its guarded block (one load latency per channel)
  if (cw + kWaveCh <= C) {
#pragma unroll
    for (int cc = 0; cc < kWaveCh; ++cc) PxN<T, PX>::store(out + ((long long)b * C + cw + cc) * hw + t.p, y[cc]);
  } else {
#pragma unroll
    for (int cc = 0; cc < kWaveCh; ++cc)
      if (cw + cc < C) PxN<T, PX>::store(out + ((long long)b * C + cw + cc) * hw + t.p, y[cc]);
  }
}

// partial[tile][c][4] = sum over the tile's pixels of dout*relu'(pre) * (1, g0, g1, g2).  Each
// lane sums its PX pixels for the wave's 8 channels (32 values), then the wave sums the 64
// lanes' values through LDS in fixed order (deterministic).
template <typename T, int PX>
__device__ __forceinline__ void dggm_bwd_block(float (*sg)[512], float4* swb, float (*sred)[64 * kRedStride], int bx,
                                               int by, const T* __restrict__ dout, const float* __restrict__ grad,
                                               const float* __restrict__ mask, long long pvs, int H, int W, int C,
                                               int h, int w, const float* __restrict__ wt,
                                               const float* __restrict__ bias, float* __restrict__ partial) {
  constexpr int TP = 64 * PX;
  const int hw = h * w, tpi = (hw + TP - 1) / TP;
  const int b = bx / tpi, p0 = (bx % tpi) * TP;
  const TileGates<PX> t = stage_gates<PX>(sg, swb, grad + b * pvs, mask + b * pvs, H, W, h, w, p0, wt, bias, C, by);
  const int lane = threadIdx.x & 63;
  const int cw = by * kBlkCh + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * kWaveCh;
  if (cw >= C) return;
  float d[kWaveCh][PX];
  if (t.valid) {
#pragma unroll
    for (int cc = 0; cc < kWaveCh; ++cc) PxN<T, PX>::load(dout + ((long long)b * C + min(cw + cc, C - 1)) * hw + t.p, d[cc]);
    __builtin_amdgcn_sched_barrier(0);  // keep the whole load batch ahead of the first use
  } else {
#pragma unroll
    for (int cc = 0; cc < kWaveCh; ++cc)
#pragma unroll
      for (int j = 0; j < PX; ++j) d[cc][j] = 0.f;
  }
  float v[4 * kWaveCh];
#pragma unroll
  for (int cc = 0; cc < kWaveCh; ++cc) {
    const int c = min(cw + cc, C - 1);
    const float4 wb = swb[c - by * kBlkCh];
    const float w0 = wb.x, w1 = wb.y, w2 = wb.z, bc = wb.w;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      const float pre = bc + w0 * t.g[0][j] + w1 * t.g[1][j] + w2 * t.g[2][j];
      const float dj = pre > 0.f ? d[cc][j] : 0.f;
      s0 += dj;
      s1 += dj * t.g[0][j];
      s2 += dj * t.g[1][j];
      s3 += dj * t.g[2][j];
    }
    v[4 * cc + 0] = s0;
    v[4 * cc + 1] = s1;
    v[4 * cc + 2] = s2;
    v[4 * cc + 3] = s3;
  }
  // wave reduction through LDS: row = lane (32 sums, stride 36 floats), then lane (idx, half)
  // adds rows half*32 .. half*32+31 of column idx; independent reads, fixed order
  float* red = sred[threadIdx.x >> 6];
#pragma unroll
  for (int q = 0; q < 8; ++q)
    *(float4*)&red[lane * kRedStride + 4 * q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
  __builtin_amdgcn_wave_barrier();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  const int idx = lane & 31, half = lane >> 5;
  float s = 0.f;
#pragma unroll
  for (int r = 0; r < 32; ++r) s += red[(half * 32 + r) * kRedStride + idx];
  s += __shfl_xor(s, 32);
  const int c = cw + (idx >> 2);
  if (lane < 32 && c < C) partial[((long long)bx * C + c) * 4 + (idx & 3)] = s;
}

// ---- up to four scales in one launch (the four backbone scales of one step): a flat block index
// is mapped onto (scale, pixel tile, channel block); the vector width PX is per scale, uniform per
// block.  Cuts three launch/drain tails per direction on the small scales.
constexpr int DGGM_MAX_SCALES = 4;
struct DggmScaleArgs {
  const void* cp1;
  const void* color;  // fwd input / bwd: dout
  void* out;
  const float* wt;
  const float* bias;
  float* partial;     // bwd
  float* dw;          // bwd outputs
  float* db;
  int C, h, w, px, nbx, blk0, tiles;
  int cp1_nhwc;       // fwd: cp1 is NHWC [B][h][w][C] (C % 8 == 0)
};
struct DggmMulti {
  DggmScaleArgs s[DGGM_MAX_SCALES];
  int n, total;
};

__device__ __forceinline__ int dggm_scale_of(const DggmMulti& m, int blk) {
  int k = 0;
#pragma unroll
  for (int i = 1; i < DGGM_MAX_SCALES; ++i)
    if (i < m.n && blk >= m.s[i].blk0) k = i;
  return k;
}

// f(std::integral_constant<int, PX>) for the scale's vector width (8, 4 or 1)
template <typename F>
__device__ __forceinline__ void dggm_with_px(int px, F&& f) {
  if (px == 8)
    f(std::integral_constant<int, 8>{});
  else if (px == 4)
    f(std::integral_constant<int, 4>{});
  else
    f(std::integral_constant<int, 1>{});
}

template <typename T>
__global__ __launch_bounds__(256) void k_dggm_fuse_fwd_multi(DggmMulti m, const float* __restrict__ grad,
                                                             const float* __restrict__ mask, long long pvs, int H,
                                                             int W) {
  __shared__ float sg[3][512];
  __shared__ float4 swb[kBlkCh];
  const int k = dggm_scale_of(m, blockIdx.x);
  const DggmScaleArgs& d = m.s[k];
  const int local = blockIdx.x - d.blk0, bx = local % d.nbx, by = local / d.nbx;
  const T* cp1 = (const T*)d.cp1;
  auto run = [&](auto has1, auto nhwc) __attribute__((always_inline)) {
    dggm_with_px(d.px, [&](auto px) __attribute__((always_inline)) {
      dggm_fwd_block<T, decltype(px)::value, decltype(has1)::value, decltype(nhwc)::value>(
          sg, swb, bx, by, decltype(has1)::value ? cp1 : nullptr, (const T*)d.color, grad, mask, pvs, H, W, d.C, d.h,
          d.w, d.wt, d.bias, (T*)d.out);
    });
  };
  if (cp1 && d.cp1_nhwc)
    run(std::true_type{}, std::true_type{});
  else if (cp1)
    run(std::true_type{}, std::false_type{});
  else
    run(std::false_type{}, std::false_type{});
}

template <typename T>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_dggm_fuse_bwd_multi(
    DggmMulti m, const float* __restrict__ grad, const float* __restrict__ mask, long long pvs, int H, int W) {
  __shared__ float sg[3][512];
  __shared__ float4 swb[kBlkCh];
  __shared__ __attribute__((aligned(16))) float sred[4][64 * kRedStride];
  const int k = dggm_scale_of(m, blockIdx.x);
  const DggmScaleArgs& d = m.s[k];
  const int local = blockIdx.x - d.blk0, bx = local % d.nbx, by = local / d.nbx;
  dggm_with_px(d.px, [&](auto px) __attribute__((always_inline)) {
    dggm_bwd_block<T, decltype(px)::value>(sg, swb, sred, bx, by, (const T*)d.color, grad, mask, pvs, H, W, d.C, d.h,
                                           d.w, d.wt, d.bias, d.partial);
  });
}

// the tile sums of every scale reduced in one launch: block = (scale, c, j); a fixed-shape tree
// over the tiles: deterministic
__global__ __launch_bounds__(256) void k_dggm_fuse_bwd_final_multi(DggmMulti m) {
  __shared__ float red[256];
  int k = 0, t = blockIdx.x;
  while (k + 1 < m.n && t >= 4 * m.s[k].C) {
    t -= 4 * m.s[k].C;
    ++k;
  }
  const DggmScaleArgs& d = m.s[k];
  float s = 0.f;
  for (int i = threadIdx.x; i < d.tiles; i += 256) s += d.partial[(long long)i * d.C * 4 + t];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x) return;
  const int c = t >> 2, j = t & 3;
  if (j == 0)
    d.db[c] = red[0];
  else
    d.dw[c * 3 + (j - 1)] = red[0];
}

int dggm_px(int h, int w) {
  const long long hw = (long long)h * w;
  return hw % 8 == 0 ? 8 : (hw % 4 == 0 ? 4 : 1);
}

// pixel tiles of one scale over the batch (h * w < 2^31)
long long dggm_tiles(int B, int h, int w) { return (long long)B * ceil_div((long long)h * w, 64 * dggm_px(h, w)); }

// The shapes, tile counts and block ranges of n scales (host arrays, n <= 4); the callers add the
// pointers.  Slots and fields a call does not use stay zero.
int dggm_multi_setup(int n, const int* C, const int* h, const int* w, int B, DggmMulti& m) {
  RGBD_REQUIRE(n >= 1 && n <= DGGM_MAX_SCALES && C && h && w, RGBD_E_ARG);
  m = DggmMulti{};
  m.n = n;
  long long blk = 0;
  for (int k = 0; k < n; ++k) {
    RGBD_REQUIRE(C[k] > 0 && h[k] > 0 && w[k] > 0 && (long long)h[k] * w[k] < (1ll << 31), RGBD_E_ARG);
    const long long nbx = dggm_tiles(B, h[k], w[k]);
    RGBD_REQUIRE(blk + nbx * ceil_div(C[k], kBlkCh) < (1ll << 31), RGBD_E_SHAPE);  // the flat grid
    DggmScaleArgs& d = m.s[k];
    d.C = C[k];
    d.h = h[k];
    d.w = w[k];
    d.px = dggm_px(h[k], w[k]);
    d.nbx = d.tiles = (int)nbx;
    d.blk0 = (int)blk;
    blk += nbx * ceil_div(C[k], kBlkCh);
  }
  m.total = (int)blk;
  return RGBD_OK;
}

}  // namespace

extern "C" {

size_t rgbd_dggm_fuse_bwd_workspace_size(int B, int C, int h, int w) {
  return align256(sizeof(float) * 4 * (size_t)C * (size_t)dggm_tiles(B, h, w));
}

size_t rgbd_dggm_fuse_bwd_multi_workspace_size(int n, const int* C_host, const int* h_host, const int* w_host,
                                               int B) {
  size_t tot = 0;
  for (int k = 0; k < n; ++k) tot += rgbd_dggm_fuse_bwd_workspace_size(B, C_host[k], h_host[k], w_host[k]);
  return tot;
}

// Scales given as host arrays (n <= 4): one launch.
int rgbd_dggm_fuse_fwd_multi(int dtype, int n, const void* const* cp1_host, int cp1_nhwc_mask,
                             const void* const* color_host, void* const* out_host, const float* const* weight_host,
                             const float* const* bias_host, const int* C_host, const int* h_host, const int* w_host,
                             const float* grad, const float* mask, long long pv_batch_stride, int B, int H, int W,
                             void* stream) {
  RGBD_REQUIRE(grad && mask && color_host && out_host && weight_host && bias_host && B > 0 && H > 0 && W > 0,
               RGBD_E_ARG);
  DggmMulti m;
  const int rc = dggm_multi_setup(n, C_host, h_host, w_host, B, m);
  if (rc) return rc;
  for (int k = 0; k < n; ++k) {
    RGBD_REQUIRE(color_host[k] && out_host[k] && weight_host[k] && bias_host[k], RGBD_E_ARG);
    m.s[k].cp1 = cp1_host ? cp1_host[k] : nullptr;
    m.s[k].cp1_nhwc = (cp1_nhwc_mask >> k) & 1;
    RGBD_REQUIRE(!m.s[k].cp1_nhwc || (C_host[k] % 8 == 0 && m.s[k].cp1), RGBD_E_SHAPE);
    m.s[k].color = color_host[k];
    m.s[k].out = out_host[k];
    m.s[k].wt = weight_host[k];
    m.s[k].bias = bias_host[k];
  }
  hipStream_t s = (hipStream_t)stream;
  TimerScope ts("dggm_fwd", s);
  if (dtype == RGBD_F32)
    k_dggm_fuse_fwd_multi<float><<<m.total, 256, 0, s>>>(m, grad, mask, pv_batch_stride, H, W);
  else if (dtype == RGBD_BF16)
    k_dggm_fuse_fwd_multi<bf16_t><<<m.total, 256, 0, s>>>(m, grad, mask, pv_batch_stride, H, W);
  else
    return RGBD_E_DTYPE;
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

// Two launches: the tile sums partial[tile][c][4] of every scale (scale k's at ws + the workspace
// sizes of the scales before it), then their reduction.
int rgbd_dggm_fuse_bwd_multi(int dtype, int n, const void* const* dout_host, const float* const* weight_host,
                             const float* const* bias_host, float* const* dweight_host, float* const* dbias_host,
                             const int* C_host, const int* h_host, const int* w_host, const float* grad,
                             const float* mask, long long pv_batch_stride, int B, int H, int W, void* ws,
                             void* stream) {
  RGBD_REQUIRE(grad && mask && dout_host && weight_host && bias_host && dweight_host && dbias_host && ws && B > 0 &&
                   H > 0 && W > 0,
               RGBD_E_ARG);
  DggmMulti m;
  const int rc = dggm_multi_setup(n, C_host, h_host, w_host, B, m);
  if (rc) return rc;
  char* p = (char*)ws;
  int nfin = 0;
  for (int k = 0; k < n; ++k) {
    RGBD_REQUIRE(dout_host[k] && weight_host[k] && bias_host[k] && dweight_host[k] && dbias_host[k], RGBD_E_ARG);
    m.s[k].color = dout_host[k];
    m.s[k].wt = weight_host[k];
    m.s[k].bias = bias_host[k];
    m.s[k].partial = (float*)p;
    m.s[k].dw = dweight_host[k];
    m.s[k].db = dbias_host[k];
    p += rgbd_dggm_fuse_bwd_workspace_size(B, C_host[k], h_host[k], w_host[k]);
    nfin += 4 * C_host[k];
  }
  hipStream_t s = (hipStream_t)stream;
  TimerScope ts("dggm_bwd", s);
  if (dtype == RGBD_F32)
    k_dggm_fuse_bwd_multi<float><<<m.total, 256, 0, s>>>(m, grad, mask, pv_batch_stride, H, W);
  else if (dtype == RGBD_BF16)
    k_dggm_fuse_bwd_multi<bf16_t><<<m.total, 256, 0, s>>>(m, grad, mask, pv_batch_stride, H, W);
  else
    return RGBD_E_DTYPE;
  k_dggm_fuse_bwd_final_multi<<<nfin, 256, 0, s>>>(m);
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

// The single-scale forms: their own argument checks and return codes, then the n = 1 case of the
// calls above (the same kernels, tile decomposition, workspace layout and reduction tree).
int rgbd_dggm_fuse_fwd(int dtype, const void* cp1, const void* color, const float* grad,
                       const float* mask, long long pv_batch_stride, int B, int H, int W, int C,
                       int h, int w, const float* weight, const float* bias, void* out,
                       void* stream) {
  RGBD_REQUIRE(color && grad && mask && weight && bias && out, RGBD_E_ARG);
  RGBD_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && h > 0 && w > 0, RGBD_E_ARG);
  RGBD_REQUIRE((long long)h * w < (1ll << 31), RGBD_E_SHAPE);
  return rgbd_dggm_fuse_fwd_multi(dtype, 1, cp1 ? &cp1 : nullptr, 0, &color, &out, &weight, &bias, &C, &h, &w, grad,
                                  mask, pv_batch_stride, B, H, W, stream);
}

int rgbd_dggm_fuse_bwd(int dtype, const void* dout, const float* grad, const float* mask,
                       long long pv_batch_stride, int B, int H, int W, int C, int h, int w,
                       const float* weight, const float* bias, float* dweight, float* dbias,
                       void* ws, void* stream) {
  RGBD_REQUIRE(dout && grad && mask && weight && bias && dweight && dbias && ws, RGBD_E_ARG);
  RGBD_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && h > 0 && w > 0, RGBD_E_ARG);
  RGBD_REQUIRE((long long)h * w < (1ll << 31), RGBD_E_SHAPE);
  return rgbd_dggm_fuse_bwd_multi(dtype, 1, &dout, &weight, &bias, &dweight, &dbias, &C, &h, &w, grad, mask,
                                  pv_batch_stride, B, H, W, ws, stream);
}

}  // extern "C"

