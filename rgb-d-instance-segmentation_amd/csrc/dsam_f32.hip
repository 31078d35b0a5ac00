// K5, float32 (the parity path): the DSAM forward / dX as one segment-form implicit GEMM
// (K = 5 segments x 9 taps x Cin, the mask bit applied per segment), and dW / db by a split-batch
// GEMM, a fixed-order combine of the splits and the channel sums of the upstream gradient.
// Launch functions at the end (dsam_common.hpp).
#include "dsam_common.hpp"

using namespace rgbd;
using namespace rgbd::k5;

namespace {

constexpr int BM = 64, BN = 64;

__global__ __launch_bounds__(256) void k_conv_igemm(ConvArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int wm = wave & 1, wn = wave >> 1;
  int py = 0, px = 0, Hc = a.Ho, Wc = a.Wo;
  if (a.transposed) {
    py = blockIdx.z >> 1;
    px = blockIdx.z & 1;
    Hc = (a.Ho - py + 1) >> 1;
    Wc = (a.Wo - px + 1) >> 1;
  }
  const long long HWc = (long long)Hc * Wc;
  const long long Mtot = (long long)a.B * HWc;
  const long long mbase = (long long)blockIdx.x * BM + wm * 32;
  const int nbase = blockIdx.y * BN + wn * 32;
  if (mbase >= Mtot) return;  // wave-uniform

  int rb[2], roy[2], rox[2];
  bool rvalid[2];
  uint32_t rcode[2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi) {
    const long long m = mbase + 16 * mi + r;
    rvalid[mi] = m < Mtot;
    const long long mm = rvalid[mi] ? m : 0;
    rb[mi] = (int)(mm / HWc);
    const int rem = (int)(mm % HWc);
    const int i = rem / Wc, j = rem % Wc;
    roy[mi] = a.transposed ? 2 * i + py : i;
    rox[mi] = a.transposed ? 2 * j + px : j;
    rcode[mi] = (a.mask_mode == MASK_DST && rvalid[mi])
                    ? a.code[((long long)rb[mi] * a.Ho + roy[mi]) * a.Wo + rox[mi]]
                    : 0xffu;
  }
  const int ntap = a.KH * a.KW;
  const long long ktot = (long long)a.nseg * ntap * a.C;
  const float* wp = (const float*)a.w;
  const float* xp = (const float*)a.x;
  bool nvalid[2];
  const float* wrow[2];
#pragma unroll
  for (int nj = 0; nj < 2; ++nj) {
    const int n = nbase + 16 * nj + r;
    nvalid[nj] = n < a.N;
    wrow[nj] = wp + (long long)(nvalid[nj] ? n : 0) * ktot + 8 * g;
  }
  f32x4 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int nj = 0; nj < 2; ++nj) acc[mi][nj] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int ky = 0; ky < a.KH; ++ky) {
    if (a.transposed && ((py + a.pad - ky) & 1)) continue;
    for (int kx = 0; kx < a.KW; ++kx) {
      if (a.transposed && ((px + a.pad - kx) & 1)) continue;
      const int tap = ky * a.KW + kx;
      const float* src[2];
      bool inb[2];
      uint32_t scode[2];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        int iy, ix;
        if (a.transposed) {
          iy = (roy[mi] + a.pad - ky) >> 1;
          ix = (rox[mi] + a.pad - kx) >> 1;
        } else {
          iy = roy[mi] * a.stride - a.pad + ky;
          ix = rox[mi] * a.stride - a.pad + kx;
        }
        inb[mi] = rvalid[mi] && iy >= 0 && iy < a.Hi && ix >= 0 && ix < a.Wi;
        const long long pix = inb[mi] ? ((long long)rb[mi] * a.Hi + iy) * a.Wi + ix : 0;
        src[mi] = xp + pix * a.C + 8 * g;
        scode[mi] = (a.mask_mode == MASK_SRC) ? (inb[mi] ? a.code[pix] : 0u) : rcode[mi];
      }
      for (int c0 = 0; c0 < a.C; c0 += 32) {
        const bool cok = c0 + 8 * g < a.C;  // C % 8 == 0: a lane's 8-chunk is all in or all out
        Frag<float> A[2];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
          if (inb[mi] && cok)
            A[mi].load(src[mi] + c0);
          else
            A[mi].zero();
        }
        for (int seg = 0; seg < a.nseg; ++seg) {
          bool keep[2] = {true, true};
          if (a.mask_mode != MASK_NONE && seg < 4) {
            keep[0] = (scode[0] >> seg) & 1u;
            keep[1] = (scode[1] >> seg) & 1u;
            if (!__any(keep[0] || keep[1])) continue;  // all-zero segment for this wave
          }
          Frag<float> As[2] = {A[0], A[1]};
          As[0].select(keep[0]);
          As[1].select(keep[1]);
          const long long koff = ((long long)seg * ntap + tap) * a.C + c0;
#pragma unroll
          for (int nj = 0; nj < 2; ++nj) {
            Frag<float> Bf;
            if (nvalid[nj] && cok)
              Bf.load(wrow[nj] + koff);
            else
              Bf.zero();
            mma(acc[0][nj], As[0], Bf);
            mma(acc[1][nj], As[1], Bf);
          }
        }
      }
    }
  }

  // epilogue: D[m = row][n = col], row = 4g + reg, col = r
  const float* res = (const float*)a.residual;
  float* onchw = (float*)a.out_nchw;
  float* onhwc = (float*)a.out_nhwc;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const long long m = mbase + 16 * mi + 4 * g + reg;
      if (m >= Mtot) continue;
      const int b = (int)(m / HWc);
      const int rem = (int)(m % HWc);
      const int i = rem / Wc, j = rem % Wc;
      const int oy = a.transposed ? 2 * i + py : i;
      const int ox = a.transposed ? 2 * j + px : j;
      int nmask = 0;
      if (a.info) nmask = a.info[b].n_masks;
#pragma unroll
      for (int nj = 0; nj < 2; ++nj) {
        const int n = nbase + 16 * nj + r;
        if (n >= a.N) continue;
        float v = acc[mi][nj][reg];
        if (a.bias4) {
          float bs = 0.f;
          for (int s = 0; s < nmask; ++s) bs += a.bias4[s * a.N + n];
          v += bs;
        }
        const long long o_nchw = (((long long)b * a.N + n) * a.Ho + oy) * a.Wo + ox;
        if (res) v = Num<float>::to_f(res[o_nchw]) + v;
        const float tv = Num<float>::from_f(v);
        if (onchw) onchw[o_nchw] = tv;
        if (onhwc) onhwc[(((long long)b * a.Ho + oy) * a.Wo + ox) * a.N + n] = tv;
      }
    }
  }
}

// ----------------------------------------------------------------------- dW
// D[o][kk] = sum_m G[m][o] * X[m][kk],  kk = (seg*9 + tap)*Cin + c,  per split z (images).
__global__ __launch_bounds__(256) void k_dsam_wgrad(const float* __restrict__ gout, const float* __restrict__ x,
                                                    const uint8_t* __restrict__ code, int B, int Cin,
                                                    int h, int w, int Cout, int splits,
                                                    float* __restrict__ partial) {
  __shared__ float Gs[64][32 + 8];   // [o][px]
  __shared__ float Xs[32][64 + 8];   // [px][kk]
  const int ho = (h + 1) / 2, wo = (w + 1) / 2;  // 3x3 s2 p1
  const int hwo = ho * wo;
  const int KK = 45 * Cin;
  const int kk0 = blockIdx.x * 64, o0 = blockIdx.y * 64, z = blockIdx.z;
  const int b0 = (int)((long long)z * B / splits), b1 = (int)((long long)(z + 1) * B / splits);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int wm = wave & 1, wn = wave >> 1;
  f32x4 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int nj = 0; nj < 2; ++nj) acc[mi][nj] = f32x4{0.f, 0.f, 0.f, 0.f};
  // staging roles
  const int go = threadIdx.x >> 2, gp = (threadIdx.x & 3) * 8;     // G: o row, 8 px
  const int xpx = threadIdx.x >> 3, xk = (threadIdx.x & 7) * 8;     // X: px row, 8 kk
  const int kk = kk0 + xk;
  const bool kk_ok = kk < KK;
  const int seg = kk_ok ? kk / (9 * Cin) : 0;
  const int tap = kk_ok ? (kk / Cin) % 9 : 0;
  const int cc = kk_ok ? kk % Cin : 0;
  const int ky = tap / 3, kx = tap % 3;
  for (int b = b0; b < b1; ++b) {
    for (int p0 = 0; p0 < hwo; p0 += 32) {
      __syncthreads();
      {  // stage G^float tile
        const int o = o0 + go;
        for (int j = 0; j < 8; ++j) {
          const int p = p0 + gp + j;
          Gs[go][gp + j] = (o < Cout && p < hwo) ? gout[((long long)b * Cout + o) * hwo + p] : (float)0;
        }
      }
      {  // stage im2col tile
        const int p = p0 + xpx;
        bool ok = kk_ok && p < hwo;
        int iy = 0, ix = 0;
        if (ok) {
          iy = 2 * (p / wo) - 1 + ky;
          ix = 2 * (p % wo) - 1 + kx;
          ok = iy >= 0 && iy < h && ix >= 0 && ix < w;
        }
        const long long pix = ((long long)b * h + iy) * w + ix;
        if (ok && seg < 4) ok = (code[pix] >> seg) & 1u;
        for (int j = 0; j < 8; ++j) Xs[xpx][xk + j] = ok ? x[pix * Cin + cc + j] : (float)0;
      }
      __syncthreads();
      Frag<float> Af[2], Bf[2];
#pragma unroll
      for (int mi = 0; mi < 2; ++mi) {
        const int o = wm * 32 + 16 * mi + r;
#pragma unroll
        for (int j = 0; j < 8; ++j) Af[mi].set(j, Num<float>::to_f(Gs[o][8 * g + j]));
      }
#pragma unroll
      for (int nj = 0; nj < 2; ++nj) {
        const int c = wn * 32 + 16 * nj + r;
#pragma unroll
        for (int j = 0; j < 8; ++j) Bf[nj].set(j, Num<float>::to_f(Xs[8 * g + j][c]));
      }
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int nj = 0; nj < 2; ++nj) mma(acc[mi][nj], Af[mi], Bf[nj]);
    }
  }
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int o = o0 + wm * 32 + 16 * mi + 4 * g + reg;
#pragma unroll
      for (int nj = 0; nj < 2; ++nj) {
        const int c = kk0 + wn * 32 + 16 * nj + r;
        if (o < Cout && c < KK) partial[((long long)z * Cout + o) * KK + c] = acc[mi][nj][reg];
      }
    }
}

__global__ void k_dsam_wgrad_final(const float* __restrict__ partial, int splits, int Cin, int Cout,
                                   float* __restrict__ dconv_w, float* __restrict__ dproj_w) {
  const long long KK = 45ll * Cin;
  const long long total = (long long)Cout * KK;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    float s = 0.f;
    for (int z = 0; z < splits; ++z) s += partial[(long long)z * total + e];  // fixed order
    const int o = (int)(e / KK);
    const int kk = (int)(e % KK);
    const int seg = kk / (9 * Cin), tap = (kk / Cin) % 9, c = kk % Cin;
    if (seg < 4)
      dconv_w[(((long long)seg * Cout + o) * Cin + c) * 9 + tap] = s;
    else
      dproj_w[((long long)o * Cin + c) * 9 + tap] = s;
  }
}

__global__ __launch_bounds__(256) void k_dsam_bias_grad(const float* __restrict__ csum, const rgbd_decomp_info* info,
                                                        int B, int Cout, int nsplit, float* __restrict__ dbias) {
  // csum [nsplit][B][Cout] channel sums (per-pixel-range partials).  One wave per (i, o): lanes
  // over (split, b) pairs, fixed-order wave tree: deterministic.
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;  // t = (i, o)
  if (t >= 4 * Cout) return;
  const int i = t / Cout, o = t % Cout;
  float s = 0.f;
  for (int q = lane; q < nsplit * B; q += 64) {
    const int b = q % B;
    if (i < info[b].n_masks) s += csum[(long long)q * Cout + o];  // conv_layers[i] used only if i < len(masks)
  }
  s = wave_sum(s);
  if (lane == 0) dbias[t] = s;
}

// batch splits of the dW GEMM: about 1024 workgroups
int dsam_wgrad_splits(int B, int Cin, int Cout) {
  const long long tiles = (long long)ceil_div(45ll * Cin, 64) * ceil_div(Cout, 64);
  int sp = (int)std::min<long long>(B, std::max<long long>(1, ceil_div(1024, tiles)));
  return sp < 1 ? 1 : sp;
}

}  // namespace

namespace rgbd::k5 {

int conv_f32(const ConvArgs& a, hipStream_t s) {
  TimerScope ts(a.transposed ? "dsam_dx" : "dsam_fwd", s);
  dim3 grid(ceil_div(conv_mmax(a), BM), ceil_div(a.N, BN), a.transposed ? 4 : 1);
  k_conv_igemm<<<grid, 256, 0, s>>>(a);
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

size_t wgrad_f32_partial_elems(int B, int Cin, int Cout) {
  return (size_t)dsam_wgrad_splits(B, Cin, Cout) * Cout * 45 * Cin;
}

int wgrad_f32(const float* gout_nchw, const float* x_nhwc, const uint8_t* code, const rgbd_decomp_info* info, int B,
              int Cin, int h, int w, int Cout, float* dconv_w, float* dproj_w, float* dbias, void* ws, hipStream_t s) {
  TimerScope ts("dsam_wgrad", s);
  float* partial = (float*)ws;
  float* csum = (float*)((char*)ws + dw_run_ws(wgrad_f32_partial_elems(B, Cin, Cout), B, Cout).csum);
  const int hwo = ((h + 1) / 2) * ((w + 1) / 2);
  const int sp = dsam_wgrad_splits(B, Cin, Cout);
  dim3 grid(ceil_div(45ll * Cin, 64), ceil_div(Cout, 64), sp);
  k_dsam_wgrad<<<grid, 256, 0, s>>>(gout_nchw, x_nhwc, code, B, Cin, h, w, Cout, sp, partial);
  k_chan_sum<float><<<B * Cout, 256, 0, s>>>(gout_nchw, hwo, csum);
  const long long total = 45ll * Cin * Cout;
  k_dsam_wgrad_final<<<(int)std::min<long long>(ceil_div(total, 256), 4096), 256, 0, s>>>(
      partial, sp, Cin, Cout, dconv_w, dproj_w);
  k_dsam_bias_grad<<<Cout, 256, 0, s>>>(csum, info, B, Cout, 1, dbias);
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

}  // namespace rgbd::k5
