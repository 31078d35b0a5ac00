// K4 (the window-ratio predictor) internals shared by ratio.hip and its stage files
// ratio_{stem,chain,conv5,f32,tail}.hip: the packed-weight layout, the tile constants the
// workspace carve needs, the BatchNorm device helpers, and the stage files' host launch functions.
// The overview of what runs when is at the top of ratio.hip.
#pragma once
#include <algorithm>

#include "mfma.hpp"
#include "timing.hpp"

namespace rgbd::rp {

constexpr int STEM_K = 160, STEM_C = 192, FUS_C = 128, ATT_C = 64, C5 = 256, C6 = 512;
// bf16 chain v2 stem: k = (c*7 + dy)*8 + dx over the 7x7 window, dx = 7 a zero pad (21 groups of 8)
constexpr int STEM_K2 = 168;
constexpr int NBN = 6;  // BN layers: scale1, scale2, scale3, fusion, fe.1, fe.5
constexpr float BN_EPS = 1e-5f;

struct Layout {  // byte offsets into the packed blob
  size_t w1, b1, w2, b2, w3, b3, w4, b4, w5, b5, w6, b6, w7, b7, w8, b8, w9, b9, w10, b10;
  size_t zero;       // 256 zero bytes
  size_t w5q;        // bf16: conv5 weights in k_rp_conv5_v4's step order
  size_t w1s;        // bf16: stem weights in the chain v2 K order
  size_t w1f, w2f;   // bf16 blobs: f32 stem (w1s order) and fusion (chain order) weights, the BN-fold sources
  size_t total;
};

inline Layout make_layout(int es) {
  Layout L;
  size_t o = 0;
  auto seg = [&](size_t bytes) {
    size_t r = o;
    o += align256(bytes);
    return r;
  };
  L.w1 = seg((size_t)STEM_C * STEM_K * es);
  L.b1 = seg(STEM_C * 4);
  L.w2 = seg((size_t)FUS_C * STEM_C * es);
  L.b2 = seg(FUS_C * 4);
  L.w3 = seg((size_t)ATT_C * FUS_C * es);
  L.b3 = seg(ATT_C * 4);
  L.w4 = seg((size_t)FUS_C * ATT_C * es);
  L.b4 = seg(FUS_C * 4);
  L.w5 = seg((size_t)C5 * 9 * FUS_C * es);
  L.b5 = seg(C5 * 4);
  L.w6 = seg((size_t)C6 * C5 * 9 * 4);
  L.b6 = seg(C6 * 4);
  L.w7 = seg(128 * 512 * 4);
  L.b7 = seg(128 * 4);
  L.w8 = seg(64 * 128 * 4);
  L.b8 = seg(64 * 4);
  L.w9 = seg(32 * 64 * 4);
  L.b9 = seg(32 * 4);
  L.w10 = seg(32 * 4);
  L.b10 = seg(4);
  L.zero = seg(256);
  L.w1s = seg(es == 2 ? (size_t)STEM_C * STEM_K2 * 2 : 0);
  L.w1f = seg(es == 2 ? (size_t)STEM_C * STEM_K2 * 4 : 0);
  L.w2f = seg(es == 2 ? (size_t)FUS_C * STEM_C * 4 : 0);
  L.w5q = seg(es == 2 ? (size_t)C5 * 9 * FUS_C * 2 : 0);
  L.total = o;
  return L;
}

// chained-operand permutation: packed position (g, e) of a 32-wide k step <-> channel
__host__ __device__ __forceinline__ int chain_perm(int g, int e) { return e < 4 ? 4 * g + e : 16 + 4 * g + (e - 4); }

struct WPtrs {  // reference-layout float32 weights (device), order of RGBD_RATIO_NW
  const float* p[RGBD_RATIO_NW];
};
struct BnPtrs {  // per BN layer: weight, bias, running_mean, running_var
  float* p[NBN * 4];
};

// ------------------------------------------------------------------ tile constants
// (the workspace carve in ratio.hip sizes its segments from them)
// float32 chain (ratio_f32.hip)
constexpr int CH_TW = 16, CH_TH = 4;                    // tile: 4 rows x 16 cols, one row per wave
// bf16 chain v2 and gate (ratio_chain.hip, ratio_conv5.hip): 8x32-pixel tiles, a row per wave
constexpr int C2W_TH = 8, C2W_TW = 32, C2W_PH = C2W_TH + 6, C2W_PW = C2W_TW + 6;
// LDS weight rows padded by 16 bytes: W1's 352-B rows are conflict-free for the ds_read_b128
// lane groups; W2/W3/W4 (400/272/144 B) are 2-way (conflict-free strides or chunk swizzles do
// not fit the LDS budget / cost more in per-lane offsets and spills than they save, measured).
constexpr int C2W_S1 = STEM_K2 + 8, C2W_S2 = STEM_C + 8, C2W_S3 = FUS_C + 8, C2W_S4 = ATT_C + 8;
constexpr int CV_TH = 4, CV_TW = 32;             // float32 conv5 (ratio_f32.hip): 128-pixel tile
constexpr int C4_TH = 16, C4_TW = 32, C4_PW = C4_TW + 2;  // conv5 v4 (ratio_conv5.hip)
constexpr int POOL_SPLIT = 16;  // row chunks per pool region
// fold: [W1' 192 x 168 bf16][W2' 128 x 192 bf16][b1' 192 f32][b2' 128 f32] (the BN folding of
// k_rp_fold and k_stem_bn)
constexpr size_t FOLD_W1 = 0, FOLD_W2 = FOLD_W1 + (size_t)STEM_C * STEM_K2 * 2;
constexpr size_t FOLD_B1 = FOLD_W2 + (size_t)FUS_C * STEM_C * 2, FOLD_B2 = FOLD_B1 + STEM_C * 4;
constexpr size_t FOLD_BYTES = FOLD_B2 + FUS_C * 4;
inline bool stem_moments_ok(int H, int W) { return H >= 8 && W >= 8; }

// conv5 v4's input (bf16): channel-quarter-major, zero-padded planes [B][4][PH][PW][32]: pixel
// (y, x) at plane row y + 1, column x + 1, PH / PW = the 16x32 tile grid + a one-pixel border, so
// every halo read of every tile is in bounds and reads zeros outside the image.
__host__ __device__ __forceinline__ int c4_ph(int H) { return (H + 15) / 16 * 16 + 2; }
__host__ __device__ __forceinline__ int c4_pw(int W) { return (W + 31) / 32 * 32 + 2; }
__host__ __device__ __forceinline__ long long c4_att_idx(int b, int q, int y, int x, int H, int W) {
  return (((long long)b * 4 + q) * c4_ph(H) + y + 1) * c4_pw(W) * 32 + (long long)(x + 1) * 32;
}

// tile index -> (image, first row, first column) with 32-bit unsigned divisions (the 64-bit
// ones cost ~150 scalar instructions per decode, twice per tile in the chain kernels)
struct TileDec {
  int b, y0, x0;
};
__device__ __forceinline__ TileDec tile_dec(unsigned t, unsigned per, unsigned tiles_x, int th, int tw) {
  const unsigned b = t / per, rem = t - b * per, ty = rem / tiles_x;
  return TileDec{(int)b, (int)ty * th, (int)(rem - ty * tiles_x) * tw};
}

// bf16 path: v_exp_f32 + v_rcp_f32 (~1 ulp each; the result is rounded to bf16).  The bf16 chain
// also writes its BN affines and statistics with explicit fmaf (the file builds with
// -ffp-contract=off for the bit-exact paths, which would split them into v_mul + v_add).
__device__ __forceinline__ float sigmoid_fast(float x) {
  return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x));
}

// ------------------------------------------------------------------ BN affine
// scale/shift per channel: eval from running stats; train from a stats slab [nslab][C][2]
// (sum, sum of squares), reduced in fixed order in double; running stats updated like torch.
// one 256-thread block per channel; thread i sums slab rows i, i+256, ... in double, then a
// fixed-shape tree reduction: deterministic for a given nslab.
// BatchNorm from the batch sums (s, q) = (sum, sum of squares) over `count` values (train) or the
// running stats (eval): per-channel affine, running stats updated like torch (unbiased variance)
struct BnVals {  // one channel's gamma, beta and running statistics, loaded ahead of its sums
  float g, b, rm, rv;
};
__device__ __forceinline__ BnVals bn_vals(const float* gamma, const float* beta, const float* run_mean,
                                          const float* run_var, int c) {
  return BnVals{gamma[c], beta[c], run_mean[c], run_var[c]};
}
__device__ __forceinline__ float2 bn_finish_v(double s, double q, double count, int training, float momentum,
                                              const BnVals& p, float* run_mean, float* run_var, int c,
                                              float2* __restrict__ affine) {
  float mean, var;
  if (training) {
    const double m = s / count;
    double v = q / count - m * m;
    if (v < 0.0) v = 0.0;
    mean = (float)m;
    var = (float)v;
    const double unb = count > 1.0 ? v * count / (count - 1.0) : v;
    run_mean[c] = (1.f - momentum) * p.rm + momentum * mean;
    run_var[c] = (1.f - momentum) * p.rv + momentum * (float)unb;
  } else {
    mean = p.rm;
    var = p.rv;
  }
  const float sc = p.g / sqrtf(var + BN_EPS);
  const float2 af = make_float2(sc, p.b - mean * sc);
  affine[c] = af;
  return af;
}
__device__ __forceinline__ float2 bn_finish(double s, double q, double count, int training, float momentum,
                                            const float* gamma, const float* beta, float* run_mean, float* run_var,
                                            int c, float2* __restrict__ affine) {
  return bn_finish_v(s, q, count, training, momentum, bn_vals(gamma, beta, run_mean, run_var, c), run_mean, run_var,
                     c, affine);
}
// the channel's parameters load with the slab rows (thread 0), the sums reduce per wave by
// shuffles, then the four wave sums in order: one barrier instead of the eight of a tree
// slab layouts: row-major [nslab][row][2] (cm = 0), or channel-major [channel][nslab][2] (cm = 1:
// the bf16 chain's phase 1 and conv5 v4 write it, so a block's reads are contiguous; the rows are
// summed in the same order either way)
__device__ __forceinline__ void bn_affine_body(const float* __restrict__ slab, int nslab, int row, int c_off, int c,
                                               double count, int training, float momentum, const float* gamma,
                                               const float* beta, float* run_mean, float* run_var,
                                               float2* __restrict__ affine, int cm = 0) {
  __shared__ double red[2][4];
  BnVals pv{};
  if (threadIdx.x == 0) pv = bn_vals(gamma, beta, run_mean, run_var, c);
  double s = 0.0, q = 0.0;
  if (training) {
    // eight slab rows per thread in flight at once, summed in the same (row) order
    int i = threadIdx.x;
    for (; i + 256 * 7 < nslab; i += 256 * 8) {
      float2 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        v[u] = *reinterpret_cast<const float2*>(
            slab + (cm ? (long long)(c_off + c) * nslab + i + 256 * u : (long long)(i + 256 * u) * row + c_off + c) * 2);
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        s += (double)v[u].x;
        q += (double)v[u].y;
      }
    }
    for (; i < nslab; i += 256) {
      const long long e = cm ? (long long)(c_off + c) * nslab + i : (long long)i * row + c_off + c;
      s += (double)slab[e * 2 + 0];
      q += (double)slab[e * 2 + 1];
    }
  }
  s = wave_sum_f64(s);
  q = wave_sum_f64(q);
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = s;
    red[1][threadIdx.x >> 6] = q;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  bn_finish_v(((red[0][0] + red[0][1]) + red[0][2]) + red[0][3], ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3],
              count, training, momentum, pv, run_mean, run_var, c, affine);
}

// zero the padding of conv5 v4's input planes (everything of [PH][PW] outside the image):
// grid (8, B * 4 planes), 16 bytes per thread and iteration (k_c4_pad_zero in ratio_conv5.hip,
// and the trailing blocks of k_stem_bn in ratio_stem.hip)
__device__ inline void c4_pad_body(bf16_t* __restrict__ att, int H, int W, int bx, int plane, int nbx) {
  const int PH = c4_ph(H), PW = c4_pw(W);
  bf16_t* pl = att + (long long)plane * PH * PW * 32;
  const int edge_rows = PH - H, side = PW - W;  // full pad rows (top + bottom), pad pixels per image row
  const long long full = (long long)edge_rows * PW * 4, part = (long long)H * side * 4;  // 16-byte chunks
  for (long long i = bx * 256 + threadIdx.x; i < full + part; i += 256LL * nbx) {
    long long px;
    if (i < full) {
      const long long c = i >> 2;
      const int rr = (int)(c / PW), cc = (int)(c % PW);
      px = (long long)(rr == 0 ? 0 : H + rr) * PW + cc;
    } else {
      const long long c = (i - full) >> 2;
      const int rr = (int)(c / side), k = (int)(c % side);
      px = (long long)(rr + 1) * PW + (k == 0 ? 0 : W + k);
    }
    *reinterpret_cast<uint4*>(pl + px * 32 + 8 * (i & 3)) = make_uint4(0u, 0u, 0u, 0u);
  }
}

inline int device_cus() {
  static int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      v = 256;
    return v > 0 ? v : 256;
  }();
  return n;
}

// ------------------------------------------------------------------ stage launch functions
// Each launches its stage's kernels on stream s and returns RGBD_OK or a HIP error code.  The
// *_grid functions are the persistent kernels' workgroup counts, which size the statistics slabs.

// ratio_stem.hip: BN affines from a statistics slab (layer = index into BnPtrs; cm: slab layout,
// see bn_affine_body), and the bf16 train route's stem moments
int bn_affine(const float* slab, int nslab, int C, double count, int training, float momentum, const BnPtrs& bn,
              int layer, float2* affine, int cm, hipStream_t s);
int bn_affine_stem(const float* slab, int nslab, double count, int training, float momentum, const BnPtrs& bn,
                   float2* aff1, hipStream_t s);
size_t stem_ws_size(int B, int H, int W);
int stem_bn_moments(const float* depth3, long long bstride, int B, int H, int W, const char* blob, const Layout& L,
                    float momentum, const BnPtrs& bn, float2* aff1, char* fold, bf16_t* att, char* ws, hipStream_t s);

// ratio_chain.hip: the bf16 chain, phase 0 | 1 | 2 (phase 2 inside the "rp_chain" timer scope)
int chain_grid_v2(int B, int H, int W, int phase = 1);
int fold_bn(const char* blob, const Layout& L, const float2* aff, int which, char* fold, hipStream_t s);
int chain_v2(int phase, const float* depth3, long long bstride, int B, int H, int W, const char* blob, const Layout& L,
             const float2* aff1, const float2* aff2, const char* fold, float* slab, bf16_t* att, hipStream_t s);

// ratio_conv5.hip: gate ("rp_chain" scope), conv5 v4 MODE 0 | 1 | 2 ("rp_conv3x3" scope), its pools
int gate(const bf16_t* fus, int B, int H, int W, const char* blob, const Layout& L, const float2* aff2, bf16_t* att,
         hipStream_t s);
int c4_pad_zero(bf16_t* att, int B, int H, int W, hipStream_t s);
long long conv4_tiles(int B, int H, int W);
int conv4_grid(int B, int H, int W);
bool conv4_pool_fused(int H, int W);
int conv5_v4(int mode, const bf16_t* att, int B, int H, int W, const char* blob, const Layout& L, const float2* aff5,
             bf16_t* y, float* out, hipStream_t s);
int pool_v4(const bf16_t* y, int B, int H, int W, const float2* aff5, float* part, hipStream_t s);
int pool_finish_v4(const float* ip, int B, int H, int W, float* pooled, hipStream_t s);

// ratio_f32.hip: the float32 parity path (phase 2 in "rp_chain", conv5 in "rp_conv3x3")
int chain_grid(int B, int H, int W);
int conv_grid(int B, int H, int W);
int chain_f32(int phase, const float* depth3, long long bstride, int B, int H, int W, const char* blob,
              const Layout& L, const float2* aff1, const float2* aff2, float* slab, float* att, hipStream_t s);
int conv3x3_f32(const float* att, int B, int H, int W, const char* blob, const Layout& L, float* y, float* slab,
                hipStream_t s);
int bn_relu_pool_f32(const float* y, int B, int H, int W, const float2* aff5, float* part, hipStream_t s);

// ratio_tail.hip: the split pools' finish, and the tail both precisions share
int pool_finish(const float* part, int B, int H, int W, float* pooled, hipStream_t s);
int tail(const float* pooled, int B, int training, float momentum, const char* blob, const Layout& L,
         const BnPtrs& bn, unsigned long long seed, unsigned long long* seed_ctr, float* feat, float* h1, float* ratio,
         hipStream_t s);

}  // namespace rgbd::rp
