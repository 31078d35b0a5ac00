// K4 stage file: the float32 parity path (xf32 MFMA): the chain k_rp_chain, conv5 k_rp_conv3x3
// and its BN + ReLU + pool k_rp_bn_relu_pool.  Overview: ratio.hip.
#include "ratio_common.hpp"

using namespace rgbd;
using namespace rgbd::rp;

namespace {

// ------------------------------------------------------------------ chain (stem, fusion, attention)
constexpr int PATCH_H = CH_TH + 6, PATCH_W = CH_TW + 6;  // 7x7 halo

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + __expf(-x)); }

__device__ __forceinline__ Frag<float> load_w(const float* base, int row, int K, int s, int g) {
  Frag<float> f;
  f.load(base + (long long)row * K + 32 * s + 8 * g);
  return f;
}

// PHASE 0: stem stats; 1: fusion stats; 2: write gated attention features (NHWC)
template <int PHASE>
__global__ __launch_bounds__(256) void k_rp_chain(const float* __restrict__ depth3, long long bstride, int B,
                                                  int H, int W, const char* __restrict__ blob, Layout L,
                                                  const float2* __restrict__ aff1, const float2* __restrict__ aff2,
                                                  float* __restrict__ slab, float* __restrict__ att) {
  __shared__ float patch[3][PATCH_H][PATCH_W];
  __shared__ short ktab[STEM_K];  // k -> (c, ky, kx) offset into patch, -1 for the zero pad
  __shared__ float st[4][STEM_C][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  constexpr int NST = PHASE == 0 ? STEM_C : FUS_C;
  for (int k = threadIdx.x; k < STEM_K; k += 256) {
    short v = -1;
    if (k < 147) {
      const int tap = k / 3, c = k % 3;
      v = (short)((c * PATCH_H + tap / 7) * PATCH_W + tap % 7);
    }
    ktab[k] = v;
  }
  for (int i = threadIdx.x; i < 4 * STEM_C * 2; i += 256) (&st[0][0][0])[i] = 0.f;
  const int tiles_x = (W + CH_TW - 1) / CH_TW, tiles_y = (H + CH_TH - 1) / CH_TH;
  const long long ntiles = (long long)B * tiles_x * tiles_y;
  const long long HW = (long long)H * W;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int b = (int)(tile / ((long long)tiles_x * tiles_y));
    const int trem = (int)(tile % ((long long)tiles_x * tiles_y));
    const int y0 = (trem / tiles_x) * CH_TH, x0 = (trem % tiles_x) * CH_TW;
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * PATCH_H * PATCH_W; i += 256) {
      const int c = i / (PATCH_H * PATCH_W), yy = (i / PATCH_W) % PATCH_H, xx = i % PATCH_W;
      const int y = y0 + yy - 3, x = x0 + xx - 3;
      (&patch[0][0][0])[i] =
          (y >= 0 && y < H && x >= 0 && x < W) ? depth3[b * bstride + c * HW + (long long)y * W + x] : 0.f;
    }
    __syncthreads();
    const int py = y0 + wave, px = x0 + r;
    const bool pvalid = py < H && px < W;
    const char* bl = opaque(blob);  // re-derived per tile: no LICM of the weight loads
    const float* w1 = (const float*)(bl + L.w1);
    const float* w2 = (const float*)(bl + L.w2);
    const float* w3 = (const float*)(bl + L.w3);
    const float* w4 = (const float*)(bl + L.w4);
    const float* b1 = (const float*)(bl + L.b1);
    const float* b2 = (const float*)(bl + L.b2);
    const float* b3 = (const float*)(bl + L.b3);
    const float* b4 = (const float*)(bl + L.b4);
    const float2* af1 = opaque(aff1);
    const float2* af2 = opaque(aff2);
    // ---- stem: D1[192 ch][16 px]
    f32x4 a1[12];
#pragma unroll
    for (int t = 0; t < 12; ++t) a1[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 5; ++s) {
      Frag<float> bfr;
      {
        float vv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int off = ktab[32 * s + 8 * g + e];
          vv[e] = off >= 0 ? (&patch[0][0][0])[off + wave * PATCH_W + r] : 0.f;
        }
        bfr.from8(vv);
      }
#pragma unroll
      for (int t = 0; t < 12; ++t) {
        // the 3x3 / 5x5 branches have all-zero weights outside k in [48,99) / [24,123)
        if (t < 4 && (s == 0 || s == 4)) continue;
        if (t >= 4 && t < 8 && s == 4) continue;
        mma(a1[t], load_w(w1, 16 * t + r, STEM_K, s, g), bfr);
        __builtin_amdgcn_sched_barrier(0);  // keep weight loads from being hoisted (VGPR budget)
      }
    }
    // z1 = a1 + b1 ; stats or BN+ReLU -> chained operand
#pragma unroll
    for (int t = 0; t < 12; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) a1[t][j] += b1[16 * t + 4 * g + j];
    if constexpr (PHASE == 0) {
#pragma unroll
      for (int t = 0; t < 12; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float v = pvalid ? a1[t][j] : 0.f, q = v * v;
          for (int o = 1; o < 16; o <<= 1) {
            v += __shfl_xor(v, o);
            q += __shfl_xor(q, o);
          }
          if (r == 0) {
            st[wave][16 * t + 4 * g + j][0] += v;
            st[wave][16 * t + 4 * g + j][1] += q;
          }
        }
      continue;
    }
    Frag<float> f1[6];
#pragma unroll
    for (int s = 0; s < 6; ++s) {
      float vv[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int t = 2 * s + (e >> 2), j = e & 3, ch = 16 * t + 4 * g + j;
        const float2 af = af1[ch];
        vv[e] = fmaxf(a1[t][j] * af.x + af.y, 0.f);
      }
      f1[s].from8(vv);
    }
    // ---- fusion: D2[128][16 px]
    f32x4 a2[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      a2[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 6; ++s) mma(a2[t], load_w(w2, 16 * t + r, STEM_C, s, g), f1[s]);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < 4; ++j) a2[t][j] += b2[16 * t + 4 * g + j];
    }
    if constexpr (PHASE == 1) {
#pragma unroll
      for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float v = pvalid ? a2[t][j] : 0.f, q = v * v;
          for (int o = 1; o < 16; o <<= 1) {
            v += __shfl_xor(v, o);
            q += __shfl_xor(q, o);
          }
          if (r == 0) {
            st[wave][16 * t + 4 * g + j][0] += v;
            st[wave][16 * t + 4 * g + j][1] += q;
          }
        }
      continue;
    }
    if constexpr (PHASE == 2) {
#pragma unroll
      for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float2 af = af2[16 * t + 4 * g + j];
          a2[t][j] = fmaxf(a2[t][j] * af.x + af.y, 0.f);  // fused = ReLU(BN(z2))
        }
      Frag<float> f2[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        float vv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) vv[e] = a2[2 * s + (e >> 2)][e & 3];
        f2[s].from8(vv);
      }
      // ---- attention 1: D3[64][16 px], ReLU
      f32x4 a3[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        a3[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 4; ++s) mma(a3[t], load_w(w3, 16 * t + r, FUS_C, s, g), f2[s]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 4; ++j) a3[t][j] = fmaxf(a3[t][j] + b3[16 * t + 4 * g + j], 0.f);
      }
      Frag<float> f3[2];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        float vv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) vv[e] = a3[2 * s + (e >> 2)][e & 3];
        f3[s].from8(vv);
      }
      // ---- attention 2 + sigmoid gate, store NHWC
      float* orow = att + ((long long)b * HW + (long long)py * W + px) * FUS_C;
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        f32x4 a4 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 2; ++s) mma(a4, load_w(w4, 16 * t + r, ATT_C, s, g), f3[s]);
        __builtin_amdgcn_sched_barrier(0);
        if (pvalid) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int ch = 16 * t + 4 * g + j;
            orow[ch] = a2[t][j] * sigmoidf_(a4[j] + b4[ch]);
          }
        }
      }
    }
  }
  if constexpr (PHASE < 2) {
    __syncthreads();
    for (int c = threadIdx.x; c < NST; c += 256)
#pragma unroll
      for (int q = 0; q < 2; ++q)
        slab[((long long)blockIdx.x * NST + c) * 2 + q] = ((st[0][c][q] + st[1][c][q]) + st[2][c][q]) + st[3][c][q];
  }
}

// ------------------------------------------------------------------ conv5: 3x3 128->256
constexpr int CV_PH = CV_TH + 2, CV_PW = CV_TW + 2;
constexpr int CV_BN = 128;                       // output channels per workgroup
constexpr int CV_CPAD = 40;                      // 32 channels + 8 pad (80-byte rows)

__global__ __launch_bounds__(256) void k_rp_conv3x3(const float* __restrict__ x, int B, int H, int W,
                                                    const char* __restrict__ blob, Layout L, float* __restrict__ y,
                                                    float* __restrict__ slab) {
  // x: NHWC [B][H][W][128]; y: NHWC [B][H][W][256]; slab: [grid][256][2] (sum, sumsq of y)
  __shared__ float patch[CV_PH * CV_PW][CV_CPAD];
  __shared__ float st[4][64][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int wm = wave & 1, wn = wave >> 1;   // wave tile: 64 px (2 tile rows) x 64 ch
  const int n0 = blockIdx.y * CV_BN + wn * 64;
  const float* w5 = (const float*)(blob + L.w5);
  const float* b5 = (const float*)(blob + L.b5);
  const int tiles_x = (W + CV_TW - 1) / CV_TW, tiles_y = (H + CV_TH - 1) / CV_TH;
  const long long ntiles = (long long)B * tiles_x * tiles_y;
  for (int i = threadIdx.x; i < 4 * 64 * 2; i += 256) (&st[0][0][0])[i] = 0.f;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int b = (int)(tile / ((long long)tiles_x * tiles_y));
    const int trem = (int)(tile % ((long long)tiles_x * tiles_y));
    const int y0 = (trem / tiles_x) * CV_TH, x0 = (trem % tiles_x) * CV_TW;
    f32x4 acc[4][4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int nj = 0; nj < 4; ++nj) acc[mi][nj] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < FUS_C; c0 += 32) {
      __syncthreads();
      // stage the 6x34 halo x 32 channels: 204 pixels x 4 chunks of 8 channels
      for (int i = threadIdx.x; i < CV_PH * CV_PW * 4; i += 256) {
        const int pp = i >> 2, q = i & 3;
        const int yy = y0 + pp / CV_PW - 1, xx = x0 + pp % CV_PW - 1;
        Frag<float> f;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W)
          f.load(x + (((long long)b * H + yy) * W + xx) * FUS_C + c0 + 8 * q);
        else
          f.zero();
        *reinterpret_cast<Frag<float>*>(&patch[pp][8 * q]) = f;
      }
      __syncthreads();
#pragma unroll 1
      for (int tap = 0; tap < 9; ++tap) {
        const int ky = tap / 3, kx = tap % 3;
        Frag<float> bf[4];
#pragma unroll
        for (int nj = 0; nj < 4; ++nj)
          bf[nj].load(w5 + (long long)(n0 + 16 * nj + r) * (9 * FUS_C) + tap * FUS_C + c0 + 8 * g);
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
          // rows of this 16-px tile: tile row (wm*2 + mi/2), cols (mi%2)*16 + r
          const int ty = wm * 2 + (mi >> 1), tx = (mi & 1) * 16 + r;
          Frag<float> af = *reinterpret_cast<const Frag<float>*>(&patch[(ty + ky) * CV_PW + tx + kx][8 * g]);
#pragma unroll
          for (int nj = 0; nj < 4; ++nj) mma(acc[mi][nj], af, bf[nj]);
        }
      }
    }
    // epilogue: y = acc + b5 (NHWC), BN partial sums
#pragma unroll
    for (int nj = 0; nj < 4; ++nj) {
      const int n = n0 + 16 * nj + r;
      const float bias = b5[n];
      float s = 0.f, q = 0.f;
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
        const int ty = wm * 2 + (mi >> 1);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int tx = (mi & 1) * 16 + 4 * g + j;
          const int yy = y0 + ty, xx = x0 + tx;
          const float v = acc[mi][nj][j] + bias;
          if (yy < H && xx < W) {
            y[(((long long)b * H + yy) * W + xx) * C5 + n] = v;
            s += v;
            q += v * v;
          }
        }
      }
      s += __shfl_xor(s, 16);
      s += __shfl_xor(s, 32);
      q += __shfl_xor(q, 16);
      q += __shfl_xor(q, 32);
      if (g == 0) {
        st[wave][16 * nj + r][0] += s;
        st[wave][16 * nj + r][1] += q;
      }
    }
  }
  __syncthreads();
  // waves (wm=0,1) with the same wn own the same 64 channels
  for (int i = threadIdx.x; i < CV_BN; i += 256) {
    const int wnn = i / 64, c = i % 64;
#pragma unroll
    for (int q = 0; q < 2; ++q)
      slab[((long long)blockIdx.x * C5 + blockIdx.y * CV_BN + i) * 2 + q] =
          st[2 * wnn][c][q] + st[2 * wnn + 1][c][q];
  }
}

// ------------------------------------------------------------------ BN + ReLU + AdaptiveAvgPool(4)
__global__ __launch_bounds__(256) void k_rp_bn_relu_pool(const float* __restrict__ y, int H, int W,
                                                         const float2* __restrict__ aff,
                                                         float* __restrict__ part) {
  // grid: (16 regions * POOL_SPLIT, B); 256 threads = 32 channel octets x 8 pixel lanes;
  // part[b][region][split][256] (fixed-order sums: deterministic)
  __shared__ float red[8][C5];
  const int b = blockIdx.y, reg = blockIdx.x / POOL_SPLIT, sp = blockIdx.x % POOL_SPLIT;
  const int i = reg / 4, j = reg % 4;
  const int oct = threadIdx.x & 31, pl = threadIdx.x >> 5;
  const int ya = (i * H) / 4, yb = ((i + 1) * H + 3) / 4, xa = (j * W) / 4, xb = ((j + 1) * W + 3) / 4;
  const int rows = yb - ya, cols = xb - xa;
  const int r0 = ya + (rows * sp) / POOL_SPLIT, r1 = ya + (rows * (sp + 1)) / POOL_SPLIT;
  float2 af[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) af[e] = aff[8 * oct + e];
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const int npx = (r1 - r0) * cols;
  for (int q = pl; q < npx; q += 8) {
    const int yy = r0 + q / cols, xx = xa + q % cols;
    Frag<float> f;
    f.load(y + (((long long)b * H + yy) * W + xx) * C5 + 8 * oct);
    float v[8];
    f.to8(v);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += fmaxf(v[e] * af[e].x + af[e].y, 0.f);
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[pl][8 * oct + e] = acc[e];
  __syncthreads();
  const int c = threadIdx.x;
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) s += red[k][c];
  part[(((long long)b * 16 + reg) * POOL_SPLIT + sp) * C5 + c] = s;
}

}  // namespace

namespace rgbd::rp {

int chain_grid(int B, int H, int W) {
  const long long nt = (long long)B * ((W + CH_TW - 1) / CH_TW) * ((H + CH_TH - 1) / CH_TH);
  return (int)std::min<long long>(nt, 2048);
}
int conv_grid(int B, int H, int W) {
  const long long nt = (long long)B * ((W + CV_TW - 1) / CV_TW) * ((H + CV_TH - 1) / CV_TH);
  return (int)std::min<long long>(nt, 512);
}

// phase 0 / 1: stem / fusion statistics -> slab; 2: the gated attention features -> att (NHWC)
int chain_f32(int phase, const float* depth3, long long bstride, int B, int H, int W, const char* blob,
              const Layout& L, const float2* aff1, const float2* aff2, float* slab, float* att, hipStream_t s) {
  const int gch = chain_grid(B, H, W);
  if (phase == 0) {
    k_rp_chain<0><<<gch, 256, 0, s>>>(depth3, bstride, B, H, W, blob, L, aff1, aff2, slab, att);
  } else if (phase == 1) {
    k_rp_chain<1><<<gch, 256, 0, s>>>(depth3, bstride, B, H, W, blob, L, aff1, aff2, slab, att);
  } else {
    TimerScope ts("rp_chain", s);
    k_rp_chain<2><<<gch, 256, 0, s>>>(depth3, bstride, B, H, W, blob, L, aff1, aff2, slab, att);
  }
  return RGBD_OK;
}

// y (NHWC) + per-workgroup BN partial sums -> slab [conv_grid][256][2]
int conv3x3_f32(const float* att, int B, int H, int W, const char* blob, const Layout& L, float* y, float* slab,
                hipStream_t s) {
  TimerScope ts("rp_conv3x3", s);
  k_rp_conv3x3<<<dim3(conv_grid(B, H, W), C5 / CV_BN), 256, 0, s>>>(att, B, H, W, blob, L, y, slab);
  return RGBD_OK;
}

int bn_relu_pool_f32(const float* y, int B, int H, int W, const float2* aff5, float* part, hipStream_t s) {
  k_rp_bn_relu_pool<<<dim3(16 * POOL_SPLIT, B), 256, 0, s>>>(y, H, W, aff5, part);
  return RGBD_OK;
}

}  // namespace rgbd::rp
