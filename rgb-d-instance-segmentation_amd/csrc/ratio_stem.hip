// K4 stage file: the BN affine kernels (k_bn_affine, k_bn_affine_stem) and the stem BN statistics
// of the bf16 train route from the moments of the depth windows (k_stem_lag, k_stem_sums,
// k_stem_s2, k_stem_bn).  Overview: ratio.hip.
#include "ratio_common.hpp"

using namespace rgbd;
using namespace rgbd::rp;

namespace {

__global__ __launch_bounds__(256) void k_bn_affine(const float* __restrict__ slab, int nslab, int row, int c_off,
                                                   int C, double count, int training, float momentum,
                                                   const float* gamma, const float* beta, float* run_mean,
                                                   float* run_var, float2* __restrict__ affine, int cm = 0) {
  if ((int)blockIdx.x >= C) return;
  bn_affine_body(slab, nslab, row, c_off, blockIdx.x, count, training, momentum, gamma, beta, run_mean, run_var, affine,
                 cm);
}
// the three stem BNs (scale1/2/3, 64 channels each, concatenated :1463) in one launch
__global__ __launch_bounds__(256) void k_bn_affine_stem(const float* __restrict__ slab, int nslab, double count,
                                                        int training, float momentum, BnPtrs bn,
                                                        float2* __restrict__ affine) {
  const int l = blockIdx.x / 64, c = blockIdx.x % 64;
  bn_affine_body(slab, nslab, STEM_C, 64 * l, c, count, training, momentum, bn.p[4 * l], bn.p[4 * l + 1],
                 bn.p[4 * l + 2], bn.p[4 * l + 3], affine + 64 * l);
}

// ------------------------------------------------------------------ stem BN statistics (bf16, train)
// The three stem BatchNorms (custom_model.py:1378-1394, 1463) need, per stem channel o, the batch
// sums  sum_p y_o(p)  and  sum_p y_o(p)^2  of  y_o(p) = b_o + sum_k W_ok x_k(p),  x(p) the 7x7x3
// window of the (bf16-rounded, zero-padded) depth planes at pixel p.  Both are moments of the
// windows:  sum_p y = N b + W S1,  sum_p y^2 = N b^2 + 2 b W S1 + W S2 W^T  with
// S1_k = sum_p x_k(p) and the Gram matrix S2_kl = sum_p x_k(p) x_l(p) (147 x 147).  S2 is a lag
// sum: for k = (c1, a), l = (c2, a + L) it equals the full-image correlation
//   F(c1, c2, L) = sum_{u1, v1} X_c1(u1, v1) X_c2(u1 + Ly, v1 + Lx)       (L in [-6, 6]^2)
// minus the anchors (u1, v1) that window offset a moves outside the image (at most 3 border rows
// and 3 border columns), so the whole Gram matrix costs 1 521 correlations instead of a stem
// convolution: 9 MFMAs per 32 pixels (k_stem_lag: D[(c1,Ly)][(c2,Lx)] += X_c1(u - Ly, v)
// X_c2(u, v + Lx) over rows u and 32-pixel blocks v, bf16 products exact, f32 accumulation per
// wave, double across waves / workgroups), the border rows / columns by its trailing workgroups, and
// k_stem_s2 / k_stem_bn assemble S2, S1 and the BN affines in double.  This replaces the former
// statistics pass over the stem (126 MFMAs per 32 pixels, 181 us per bench step).
constexpr int SL_R = 32, SL_CW = 256, SL_PADL = 8;          // B rows per band, columns per chunk
constexpr int SL_ROWS = SL_R + 12, SL_LD = SL_CW + 2 * SL_PADL;
constexpr int SL_NL = 39, SL_NF = SL_NL * SL_NL;             // (channel, lag) per side; correlations
constexpr int SL_REC = SL_NF + 3;                            // + the three plane sums
constexpr size_t SL_SMEM = (size_t)3 * SL_ROWS * SL_LD * 2;
constexpr int SL_GRP = 3 * SL_ROWS * (SL_LD / 4), SL_GPT = (SL_GRP + 511) / 512;  // 4-pixel groups staged
static_assert(SL_GPT % 6 == 0, "k_stem_lag staging rounds");
static_assert(SL_SMEM >= 8 * SL_NF * sizeof(float) + 8 + 24 * sizeof(double), "k_stem_lag: LDS reused for the wave reduction");
constexpr int SF_CH = 64;                                    // stem_frame_body: pixels per chunk
constexpr int SF_T = 351, SF_REC = SF_T * 13 + 9;            // sums per (kind, image, chunk)
constexpr int SF_THR = 512;  // >= SF_T + 9 + 27: the sum threads, the plain sums, the plain corner values
constexpr int SF_AL = SF_CH + 12, SF_N = 3 * 15 * SF_AL, SF_PT = (SF_N + SF_THR - 1) / SF_THR;
static_assert(SF_THR >= SF_T + 9 + 27 && SF_THR == 512, "stem_frame_body thread roles (k_stem_lag workgroups)");
static_assert(SL_SMEM >= sizeof(float) * 3 * 15 * SF_AL, "stem_frame_body strip in k_stem_lag LDS");
constexpr int SC_REC = SF_T * 39 + 27;                       // corner cells per (row kind, side, image)

struct StemGeom {
  int nband, ncol, nwg, nfr_row, nfr_col, mx;  // lag workgroups; frame chunks per row / col kind
};
inline StemGeom stem_geom(int B, int H, int W) {
  StemGeom g;
  g.nband = ceil_div(H, SL_R);
  g.ncol = ceil_div(W, SL_CW);
  g.nwg = B * g.nband * g.ncol;
  g.nfr_row = ceil_div(W, SF_CH);
  g.nfr_col = ceil_div(H, SF_CH);
  g.mx = std::max(g.nfr_row, g.nfr_col);
  return g;
}
// The row-kind chunk that writes the right corner cells: the one holding anchor column W - 3.
// Its strip (columns a0 - 6 .. a0 + SF_CH + 5) then covers every in-image column the three
// right anchors' lag windows reach (W - 9 .. W - 1); the last chunk does not when it holds
// fewer than three columns (W % 64 in {1, 2}).
__host__ __device__ __forceinline__ int stem_right_chunk(int W) { return (W - 3) / SF_CH; }

// bf16-rounded depth value (c, y, x) of image b, 0 outside: the load always reads an in-range
// element (clamped) and the value is selected after it, so loads issued together stay in flight
__device__ __forceinline__ float stem_ld(const float* __restrict__ depth3, long long bstride, long long HW, int b, int c,
                                         int H, int W, int y, int x) {
  return depth3[b * bstride + c * HW + (long long)min(max(y, 0), H - 1) * W + min(max(x, 0), W - 1)];
}
__device__ __forceinline__ float stem_sel(float v, int H, int W, int y, int x) {
  return (y >= 0 && y < H && x >= 0 && x < W) ? bf16_to_f32(f32_to_bf16(v)) : 0.f;
}

// Border rows / columns of every image: for the anchors of the three top (bottom) rows, per
// (c1, c2, Ly) and anchor row j the 13 row sums over Lx of X_c1(u1, v) X_c2(u1 + Ly, v + Lx)
// over this chunk's 64 columns; the column kinds likewise with the roles of the axes swapped; plus
// the plain sums of X_c over the anchor rows / columns.  Workgroup = (chunk, kind, image), kind 0
// top rows, 1 bottom rows, 2 left columns, 3 right columns: out [kind][image][chunk][SF_REC] f32
// (a kind's chunks past its own count write zeros).  The row kinds' first / last chunk also write
// the corner cells of the three left / right columns: cells [row kind][side][image][SC_REC] =
// the products [t][Lx][column] and the plain values [c][row][column].
// (run by the trailing workgroups of k_stem_lag: wid = (image * 4 + kind) * mx + chunk)
__device__ __forceinline__ void stem_frame_body(const float* __restrict__ depth3, long long bstride, int B, int H, int W,
                                                int nfr_row, int nfr_col, float* __restrict__ out,
                                                float* __restrict__ cells, int wid, char* smem) {
  float(*S)[15][SF_AL] = reinterpret_cast<float(*)[15][SF_AL]>(smem);  // strip: 15 lines across, 64 + 12 along
  const int mx0 = max(nfr_row, nfr_col);
  const int chunk = wid % mx0, kind = (wid / mx0) % 4, b = wid / (4 * mx0);
  const bool rows = kind < 2;
  const int nch = rows ? nfr_row : nfr_col, mx = max(nfr_row, nfr_col);
  float* o = out + (((long long)kind * B + b) * mx + chunk) * SF_REC;
  if (chunk >= nch) {
    for (int i = threadIdx.x; i < SF_REC; i += SF_THR) o[i] = 0.f;
    return;
  }
  const long long HW = (long long)H * W;
  const int a0 = chunk * SF_CH;                                      // first anchor along the strip
  const int line0 = kind == 0 ? 0 : (kind == 1 ? H - 3 : (kind == 2 ? 0 : W - 3));  // first anchor line
  float pre[SF_PT];
#pragma unroll
  for (int k = 0; k < SF_PT; ++k) {
    const int i = min((int)threadIdx.x + SF_THR * k, SF_N - 1);
    const int c = i / (15 * SF_AL), li = (i / SF_AL) % 15, al = i % SF_AL;
    const int ln = line0 - 6 + li, at = a0 - 6 + al;                // across, along
    pre[k] = rows ? stem_ld(depth3, bstride, HW, b, c, H, W, ln, at) : stem_ld(depth3, bstride, HW, b, c, H, W, at, ln);
  }
#pragma unroll
  for (int k = 0; k < SF_PT; ++k) {
    const int i = threadIdx.x + SF_THR * k;
    if (i < SF_N) {
      const int c = i / (15 * SF_AL), li = (i / SF_AL) % 15, al = i % SF_AL;
      const int ln = line0 - 6 + li, at = a0 - 6 + al;
      S[c][li][al] = rows ? stem_sel(pre[k], H, W, ln, at) : stem_sel(pre[k], H, W, at, ln);
    }
  }
  __syncthreads();
  const int along_n = rows ? W : H;
  const int nal = min(SF_CH, along_n - a0);
  const int t = threadIdx.x;
  if (t < SF_T) {  // t = ((c1 * 3 + c2) * 13 + s1) * 3 + j: s1 the across lag, 13 along lags
    const int j = t % 3, s1 = (t / 3) % 13, c2 = (t / 39) % 3, c1 = t / 117;
    float acc[13];
#pragma unroll
    for (int q = 0; q < 13; ++q) acc[q] = 0.f;
    float win[13];
#pragma unroll
    for (int q = 0; q < 13; ++q) win[q] = S[c2][j + s1][q];  // along positions a - 6 .. a + 6 of a = 0
    for (int a = 0; a < nal; ++a) {
      const float x1 = S[c1][6 + j][6 + a];
#pragma unroll
      for (int q = 0; q < 13; ++q) acc[q] = __builtin_fmaf(x1, win[q], acc[q]);
#pragma unroll
      for (int q = 0; q < 12; ++q) win[q] = win[q + 1];
      win[12] = S[c2][j + s1][min(a + 13, SF_AL - 1)];
    }
#pragma unroll
    for (int q = 0; q < 13; ++q) o[t * 13 + q] = acc[q];
    if (rows) {  // corner cells: the three left (first chunk) / right anchor columns
#pragma unroll
      for (int side = 0; side < 2; ++side) {
        if (chunk != (side == 0 ? 0 : stem_right_chunk(W))) continue;
        float* cl = cells + (((long long)kind * 2 + side) * B + b) * SC_REC;
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) {
          const int a = side == 0 ? ci : W - 3 + ci - a0;
          const float x1 = S[c1][6 + j][6 + a];
          // strip index a + q = column a0 + a + q - 6; past the strip's end the column is >= W (0)
#pragma unroll
          for (int q = 0; q < 13; ++q) cl[(t * 13 + q) * 3 + ci] = a + q < SF_AL ? x1 * S[c2][j + s1][a + q] : 0.f;
        }
      }
    }
  } else if (t < SF_T + 9) {  // plain sums of X_c over anchor line j
    const int c = (t - SF_T) / 3, j = (t - SF_T) % 3;
    float s = 0.f;
    for (int a = 0; a < nal; ++a) s += S[c][6 + j][6 + a];
    o[SF_T * 13 + c * 3 + j] = s;
  } else if (rows && t < SF_T + 9 + 27) {  // plain corner values [c][row][column]
    const int e = t - SF_T - 9, c = e / 9, j = (e / 3) % 3, ci = e % 3;
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      if (chunk != (side == 0 ? 0 : stem_right_chunk(W))) continue;
      const int a = side == 0 ? ci : W - 3 + ci - a0;
      cells[(((long long)kind * 2 + side) * B + b) * SC_REC + SF_T * 39 + e] = S[c][6 + j][6 + a];
    }
  }
}

// Diagnostics (rgbd_debug_stem_lag_stamps, diagnostic build only): every workgroup's waves record
// s_memtime at: kernel entry, window staged (after the barrier), lag loop done, waves joined,
// correlations written, plane sums written: stamps[(wg * 8 + wave) * 6 + point].
__device__ unsigned long long* g_sl_stamps = nullptr;
[[maybe_unused]] static bool sl_stamps_on = false;
[[maybe_unused]] __device__ __forceinline__ void sl_stamp(long long idx) {
  __builtin_amdgcn_sched_barrier(0);
  const unsigned long long t = __builtin_amdgcn_s_memtime();
  if ((threadIdx.x & 63) == 0) g_sl_stamps[idx] = t;
  __builtin_amdgcn_sched_barrier(0);
}

// grid: the nwg lag workgroups, then 4 * B * mx border workgroups (stem_frame_body), which fill
// the CU slots the lag workgroups leave free instead of following them in a second launch
template <bool STAMPS = false>
__global__ __launch_bounds__(512) void k_stem_lag(const float* __restrict__ depth3, long long bstride, int B, int H,
                                                  int W, int nband, int ncol, double* __restrict__ part, int nfr_row,
                                                  int nfr_col, float* __restrict__ fch, float* __restrict__ cells) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  if ((int)blockIdx.x >= B * nband * ncol) {
    stem_frame_body(depth3, bstride, B, H, W, nfr_row, nfr_col, fch, cells, (int)blockIdx.x - B * nband * ncol, smem);
    return;
  }
  const long long sbase = ((long long)blockIdx.x * 8 + (threadIdx.x >> 6)) * 6;
  if constexpr (STAMPS) sl_stamp(sbase + 0);
  bf16_t* X = (bf16_t*)smem;  // [3][SL_ROWS][SL_LD]: rows u0-6 .., columns cv0-8 ..
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int wg = blockIdx.x, b = wg / (nband * ncol), rem = wg % (nband * ncol);
  const int u0 = (rem / ncol) * SL_R, cv0 = (rem % ncol) * SL_CW;
  const long long HW = (long long)H * W;
  float tsum[3] = {0.f, 0.f, 0.f};
  // the 4-pixel groups in rounds of SL_RND: a round's loads are issued together, then converted
  // (16-byte loads where rows are aligned: the groups then never straddle the image's right edge)
  const bool vec = (W & 3) == 0 && (bstride & 3) == 0 && ((uintptr_t)depth3 & 15) == 0;
  auto put = [&](int i, float4 q) {
    const int c = i / (SL_ROWS * (SL_LD / 4)), rr = (i / (SL_LD / 4)) % SL_ROWS, cc = 4 * (i % (SL_LD / 4));
    const int yy = u0 - 6 + rr, xx = cv0 - SL_PADL + cc;
    const float v0 = stem_sel(q.x, H, W, yy, xx), v1 = stem_sel(q.y, H, W, yy, xx + 1);
    const float v2 = stem_sel(q.z, H, W, yy, xx + 2), v3 = stem_sel(q.w, H, W, yy, xx + 3);
    *reinterpret_cast<uint2*>(X + (c * SL_ROWS + rr) * SL_LD + cc) = make_uint2(pack_bf16x2(v0, v1), pack_bf16x2(v2, v3));
    // the plane sums over this workgroup's own pixels (rows [u0, u0+R), columns [cv0, cv0+CW))
    if (rr >= 6 && rr < 6 + SL_R && cc >= SL_PADL && cc < SL_PADL + SL_CW) tsum[c] += (v0 + v1) + (v2 + v3);
  };
  constexpr int SL_RND = 6;
  for (int k0 = 0; k0 < SL_GPT; k0 += SL_RND) {
    float4 q[SL_RND];
    if (vec) {
#pragma unroll
      for (int k = 0; k < SL_RND; ++k) {
        const int i = min(tid + 512 * (k0 + k), SL_GRP - 1);
        const int c = i / (SL_ROWS * (SL_LD / 4)), rr = (i / (SL_LD / 4)) % SL_ROWS, cc = 4 * (i % (SL_LD / 4));
        const int yy = u0 - 6 + rr, xx = cv0 - SL_PADL + cc;
        q[k] = *reinterpret_cast<const float4*>(depth3 + b * bstride + c * HW + (long long)min(max(yy, 0), H - 1) * W +
                                                min(max(xx, 0), W - 4));
      }
    } else {
#pragma unroll
      for (int k = 0; k < SL_RND; ++k) {
        const int i = min(tid + 512 * (k0 + k), SL_GRP - 1);
        const int c = i / (SL_ROWS * (SL_LD / 4)), rr = (i / (SL_LD / 4)) % SL_ROWS, cc = 4 * (i % (SL_LD / 4));
        const int yy = u0 - 6 + rr, xx = cv0 - SL_PADL + cc;
        q[k] = make_float4(stem_ld(depth3, bstride, HW, b, c, H, W, yy, xx),
                           stem_ld(depth3, bstride, HW, b, c, H, W, yy, xx + 1),
                           stem_ld(depth3, bstride, HW, b, c, H, W, yy, xx + 2),
                           stem_ld(depth3, bstride, HW, b, c, H, W, yy, xx + 3));
      }
    }
#pragma unroll
    for (int k = 0; k < SL_RND; ++k) {
      const int i = tid + 512 * (k0 + k);
      if (i < SL_GRP) put(i, q[k]);
    }
  }
  __syncthreads();
  if constexpr (STAMPS) sl_stamp(sbase + 1);
  // per-lane fragment bases: A rows m = (c1, Ly), B columns n = (c2, Lx); m, n >= 39 are zero
  int abase[3], bbase[3];
  bool aval[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int m = 16 * i + r;
    aval[i] = m < SL_NL;
    const int c1 = aval[i] ? m / 13 : 0, ly = aval[i] ? m % 13 - 6 : 0;
    abase[i] = (c1 * SL_ROWS + 6 - ly) * SL_LD + SL_PADL + 8 * g;     // + ur * SL_LD + (v0 - cv0)
    bbase[i] = (c1 * SL_ROWS + 6) * SL_LD + SL_PADL + 8 * g + ly;     // (c2, Lx) decode as (c1, ly)
  }
  f32x4 acc[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nrow = min(SL_R, H - u0), nvb = (min(SL_CW, W - cv0) + 31) / 32;
  const uint32_t* Xw = reinterpret_cast<const uint32_t*>(X);
  for (int it = wave; it < nrow * nvb; it += 8) {
    const int ur = it / nvb, off = ur * SL_LD + 32 * (it % nvb);
    Frag<bf16_t> fa[3], fb[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      fa[i].v = *reinterpret_cast<const uint4*>(X + abase[i] + off);
      if (!aval[i]) fa[i].zero();
      const int e = bbase[i] + off, w0 = e >> 1;
      const uint32_t sh = (e & 1) * 2;
      const uint32_t x0 = Xw[w0], x1 = Xw[w0 + 1], x2 = Xw[w0 + 2], x3 = Xw[w0 + 3], x4 = Xw[w0 + 4];
      fb[i].v = make_uint4(__builtin_amdgcn_alignbyte(x1, x0, sh), __builtin_amdgcn_alignbyte(x2, x1, sh),
                           __builtin_amdgcn_alignbyte(x3, x2, sh), __builtin_amdgcn_alignbyte(x4, x3, sh));
      if (!aval[i]) fb[i].zero();
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) mma(acc[i][j], fa[i], fb[j]);
  }
  if constexpr (STAMPS) sl_stamp(sbase + 2);
  // the 8 waves' tiles summed in double, in wave order: every wave parks its f32 tile in LDS
  // (8 x 1 521 floats), then each correlation is summed by one thread
  __syncthreads();
  if constexpr (STAMPS) sl_stamp(sbase + 3);
  float* redf = (float*)smem;  // [8 wave][SL_NF]
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int m = 16 * i + 4 * g + e, n = 16 * j + r;
        if (m < SL_NL && n < SL_NL) redf[wave * SL_NF + m * SL_NL + n] = acc[i][j][e];
      }
  // plane sums: per wave in double (lane order fixed by the butterfly), parked after the tiles
  double* wsum = (double*)(smem + 8 * SL_NF * sizeof(float) + 8);  // [8 wave][3], 8-byte aligned
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double v = (double)tsum[c];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0) wsum[wave * 3 + c] = v;
  }
  __syncthreads();
  double* out = part + (long long)wg * SL_REC;
  for (int i = tid; i < SL_NF; i += 512) {
    double t = (double)redf[i];
#pragma unroll
    for (int w = 1; w < 8; ++w) t += (double)redf[w * SL_NF + i];
    out[i] = t;
  }
  if (tid < 3) {
    double t = wsum[tid];
#pragma unroll
    for (int w = 1; w < 8; ++w) t += wsum[w * 3 + tid];
    out[SL_NF + tid] = t;
  }
  if constexpr (STAMPS) sl_stamp(sbase + 4);
  if constexpr (STAMPS) sl_stamp(sbase + 5);
}

// dst[s][e] = sum_k src[s * seg_stride + k * stride + e] (k < n, fixed order: 16 groups of every
// 16th k, then the groups in order): workgroup = 16 consecutive elements x 16 groups.
template <typename T>
__device__ __forceinline__ void stem_sum_body(const T* __restrict__ src, int n, long long stride, long long seg_stride,
                                              int seg_len, double* __restrict__ dst, int bx, int s,
                                              double (*red)[17]) {
  const int el = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const int e = bx * 16 + el;
  double acc = 0.0;
  if (e < seg_len) {
    const T* p = src + s * seg_stride + e;
    int k = grp;
    for (; k + 112 < n; k += 128) {  // eight loads in flight, added in k order
      double a[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) a[u] = (double)p[(k + 16 * u) * stride];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += a[u];
    }
    for (; k < n; k += 16) acc += (double)p[k * stride];
  }
  red[grp][el] = acc;
  __syncthreads();
  if (grp == 0 && e < seg_len) {
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) t += red[q][el];
    dst[(long long)s * seg_len + e] = t;
  }
}

// The three reductions of the stem moments in one launch (1-D grid): the lag partials -> F
// (double), the border chunks -> fr [kind] and the corner cells -> ce [row kind][side] (float).
struct StemSums {
  const double* part;
  const float *fch, *cells;
  double *F, *fr, *ce;
  int nwg, nfch, B;
};
constexpr int SS_B0 = (SL_REC + 15) / 16, SS_B1 = 4 * ((SF_REC + 15) / 16), SS_B2 = 4 * ((SC_REC + 15) / 16);
__global__ __launch_bounds__(256) void k_stem_sums(const StemSums a) {
  __shared__ double red[16][17];
  int bx = blockIdx.x;
  if (bx < SS_B0) {
    stem_sum_body<double>(a.part, a.nwg, SL_REC, 0, SL_REC, a.F, bx, 0, red);
    return;
  }
  bx -= SS_B0;
  if (bx < SS_B1) {
    const int per = SS_B1 / 4;
    stem_sum_body<float>(a.fch, a.nfch, SF_REC, (long long)a.nfch * SF_REC, SF_REC, a.fr, bx % per, bx / per, red);
    return;
  }
  bx -= SS_B1;
  const int per = SS_B2 / 4;
  stem_sum_body<float>(a.cells, a.B, SC_REC, (long long)a.B * SC_REC, SC_REC, a.ce, bx % per, bx / per, red);
}

// S2 [147][147] and S1 [147] (k = c * 49 + ay * 7 + ax, the window offset a = (ay, ax) of
// channel c) over the batch, double: thread per (k, l), the extra 147 threads S1.  fr [kind][SF_REC]
// and ce [row kind][side][SC_REC] are already summed over the images.
__global__ __launch_bounds__(256) void k_stem_s2(const double* __restrict__ F, const double* __restrict__ fr,
                                                 const double* __restrict__ ce, double* __restrict__ S2,
                                                 double* __restrict__ S1) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 147 * 147 + 147) return;
  const bool is_s1 = i >= 147 * 147;
  const int k = is_s1 ? i - 147 * 147 : i / 147, l = is_s1 ? k : i % 147;
  const int c1 = k / 49, ay = (k % 49) / 7, ax = k % 7;
  const int c2 = l / 49, by = (l % 49) / 7, bx = l % 7;
  const int ly = by - ay, lx = bx - ax;
  // excluded anchor rows / columns of offset a: top j < ay - 3, or bottom j >= ay (j = 0..2)
  const int rkind = ay > 3 ? 0 : 1, rlo = ay > 3 ? 0 : ay, rhi = ay > 3 ? ay - 3 : (ay < 3 ? 3 : 0);
  const int ckind = ax > 3 ? 2 : 3, clo = ax > 3 ? 0 : ax, chi = ax > 3 ? ax - 3 : (ax < 3 ? 3 : 0);
  const double* rk = fr + (long long)rkind * SF_REC;
  const double* ck = fr + (long long)ckind * SF_REC;
  const double* cc = ce + ((long long)rkind * 2 + (ckind - 2)) * SC_REC;
  const int trow = ((c1 * 3 + c2) * 13 + ly + 6) * 3, tcol = ((c1 * 3 + c2) * 13 + lx + 6) * 3;
  // every load in flight together (j = 0..2 index valid rows whatever the bounds; the loops over
  // the data-dependent bounds waited for each load in turn), applied in the same order as before
  double s = is_s1 ? F[SL_NF + c1] : F[(c1 * 13 + ly + 6) * SL_NL + c2 * 13 + lx + 6];
  double rv[3], cv[3], xv[3][3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    rv[j] = is_s1 ? rk[SF_T * 13 + c1 * 3 + j] : rk[(trow + j) * 13 + lx + 6];
    cv[j] = is_s1 ? ck[SF_T * 13 + c1 * 3 + j] : ck[(tcol + j) * 13 + ly + 6];
#pragma unroll
    for (int jc = 0; jc < 3; ++jc)
      xv[j][jc] = is_s1 ? cc[SF_T * 39 + (c1 * 3 + j) * 3 + jc] : cc[((trow + j) * 13 + lx + 6) * 3 + jc];
  }
#pragma unroll
  for (int j = 0; j < 3; ++j)
    if (j >= rlo && j < rhi) s -= rv[j];
#pragma unroll
  for (int j = 0; j < 3; ++j)
    if (j >= clo && j < chi) s -= cv[j];
#pragma unroll
  for (int jr = 0; jr < 3; ++jr)  // corners: excluded in both, subtracted twice
#pragma unroll
    for (int jc = 0; jc < 3; ++jc)
      if (jr >= rlo && jr < rhi && jc >= clo && jc < chi) s += xv[jr][jc];
  if (is_s1)
    S1[k] = s;
  else
    S2[i] = s;
}

// Per stem channel o (one block each): sum y = N b + w.S1, sum y^2 = N b^2 + 2 b w.S1 + w S2 w^T,
// then the BatchNorm of bn_affine_body (train mode) from the double sums, and the block folds
// its affine into W1' / b1' row o as k_rp_fold (which 1) does.  Blocks STEM_C .. STEM_C + 32 B - 1
// zero conv5 v4's input padding (k_c4_pad_zero's work: grid (8, 4 B) flattened), so neither
// small kernel is a launch of its own on the predictor's critical path.
__global__ __launch_bounds__(256) void k_stem_bn(const double* __restrict__ S2, const double* __restrict__ S1,
                                                 const char* __restrict__ blob, Layout L, double count, float momentum,
                                                 BnPtrs bn, float2* __restrict__ affine, char* __restrict__ fold,
                                                 bf16_t* __restrict__ att, int H, int W) {
  if ((int)blockIdx.x >= STEM_C) {  // block-uniform
    const int p = (int)blockIdx.x - STEM_C;
    c4_pad_body(att, H, W, p % 8, p / 8, 8);
    return;
  }
  __shared__ double red[2][256];
  __shared__ double w[147];
  __shared__ float2 s_aff;
  const int o = blockIdx.x, t = threadIdx.x;
  const bf16_t* w1s = (const bf16_t*)(blob + L.w1s);
  // the fold's source row, loaded now (in flight through the reduction)
  const float wf = t < STEM_K2 ? ((const float*)(blob + L.w1f))[(size_t)o * STEM_K2 + t] : 0.f;
  const float bf = ((const float*)(blob + L.b1))[o];
  if (t < 147) w[t] = (double)bf16_to_f32(w1s[o * STEM_K2 + ((t / 49) * 7 + (t % 49) / 7) * 8 + t % 7]);
  __syncthreads();
  double a = 0.0, q = 0.0;
  if (t < 147) {
    a = w[t] * S1[t];
    // S2 symmetric: coalesced rows.  49 rows per batch in flight together, summed in row order
    // (seven loads per round trip made the 147 serial L2 round trips most of the kernel)
    for (int l0 = 0; l0 < 147; l0 += 49) {
      double sv[49];
#pragma unroll
      for (int u = 0; u < 49; ++u) sv[u] = S2[(l0 + u) * 147 + t];
#pragma unroll
      for (int u = 0; u < 49; ++u) q += w[l0 + u] * sv[u];
    }
    q *= w[t];
  }
  red[0][t] = a;
  red[1][t] = q;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) {
      red[0][t] += red[0][t + s];
      red[1][t] += red[1][t + s];
    }
    __syncthreads();
  }
  if (t == 0) {
    const double bias = (double)bf;
    const double sy = count * bias + red[0][0];
    const double sq = count * bias * bias + 2.0 * bias * red[0][0] + red[1][0];
    const int l = o / 64, c = o % 64;
    s_aff = bn_finish(sy, sq, count, 1, momentum, bn.p[4 * l], bn.p[4 * l + 1], bn.p[4 * l + 2], bn.p[4 * l + 3], c,
                      affine + 64 * l);
  }
  __syncthreads();
  // BN1 -> W1', b1' (k_rp_fold's arithmetic)
  const float2 af = s_aff;
  if (t < STEM_K2) ((bf16_t*)(fold + FOLD_W1))[(size_t)o * STEM_K2 + t] = f32_to_bf16(wf * af.x);
  if (t == 0) ((float*)(fold + FOLD_B1))[o] = __builtin_fmaf(bf, af.x, af.y);
}

struct StemWs {
  size_t part, fchunks, cells, F, fr, ce, S2, S1, total;
};
inline StemWs stem_ws(int B, int H, int W) {
  const StemGeom g = stem_geom(B, H, W);
  StemWs s;
  size_t o = 0;
  auto seg = [&](size_t bytes) {
    size_t r = o;
    o += align256(bytes);
    return r;
  };
  s.part = seg((size_t)g.nwg * SL_REC * sizeof(double));
  s.fchunks = seg((size_t)4 * B * g.mx * SF_REC * sizeof(float));
  s.cells = seg((size_t)4 * B * SC_REC * sizeof(float));
  s.F = seg(SL_REC * sizeof(double));
  s.fr = seg((size_t)4 * SF_REC * sizeof(double));
  s.ce = seg((size_t)4 * SC_REC * sizeof(double));
  s.S2 = seg(147 * 147 * sizeof(double));
  s.S1 = seg(147 * sizeof(double));
  s.total = o;
  return s;
}

}  // namespace

namespace rgbd::rp {

int bn_affine(const float* slab, int nslab, int C, double count, int training, float momentum, const BnPtrs& bn,
              int layer, float2* affine, int cm, hipStream_t s) {
  float* const* p = bn.p + 4 * layer;
  k_bn_affine<<<C, 256, 0, s>>>(slab, nslab, C, 0, C, count, training, momentum, p[0], p[1], p[2], p[3], affine, cm);
  return RGBD_OK;
}

// the three stem BNs (scale1/2/3, 64 channels each, concatenated :1463)
int bn_affine_stem(const float* slab, int nslab, double count, int training, float momentum, const BnPtrs& bn,
                   float2* aff1, hipStream_t s) {
  k_bn_affine_stem<<<STEM_C, 256, 0, s>>>(slab, nslab, count, training, momentum, bn, aff1);
  return RGBD_OK;
}

size_t stem_ws_size(int B, int H, int W) { return stem_ws(B, H, W).total; }

// the moments of every window and the stem BN affines (aff1) + running stats, train mode
int stem_bn_moments(const float* depth3, long long bstride, int B, int H, int W, const char* blob, const Layout& L,
                    float momentum, const BnPtrs& bn, float2* aff1, char* fold, bf16_t* att, char* ws, hipStream_t s) {
  const StemGeom g = stem_geom(B, H, W);
  const StemWs w = stem_ws(B, H, W);
  double* part = (double*)(ws + w.part);
  float* fch = (float*)(ws + w.fchunks);
  float* cells = (float*)(ws + w.cells);
  double* F = (double*)(ws + w.F);
  double* fr = (double*)(ws + w.fr);
  double* ce = (double*)(ws + w.ce);
  double* S2 = (double*)(ws + w.S2);
  double* S1 = (double*)(ws + w.S1);
  static const hipError_t attr =
      hipFuncSetAttribute((const void*)k_stem_lag<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SL_SMEM);
  if (attr != hipSuccess) return (int)attr;
  const int nall = g.nwg + 4 * B * g.mx;
#ifdef RGBD_DIAG
  if (sl_stamps_on) {
    static const hipError_t dattr =
        hipFuncSetAttribute((const void*)k_stem_lag<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SL_SMEM);
    (void)dattr;
    k_stem_lag<true><<<nall, 512, SL_SMEM, s>>>(depth3, bstride, B, H, W, g.nband, g.ncol, part, g.nfr_row, g.nfr_col,
                                               fch, cells);
  } else
#endif
    k_stem_lag<false><<<nall, 512, SL_SMEM, s>>>(depth3, bstride, B, H, W, g.nband, g.ncol, part, g.nfr_row,
                                                g.nfr_col, fch, cells);
  StemSums ss{part, fch, cells, F, fr, ce, g.nwg, B * g.mx, B};
  k_stem_sums<<<SS_B0 + SS_B1 + SS_B2, 256, 0, s>>>(ss);
  k_stem_s2<<<ceil_div(147 * 147 + 147, 256), 256, 0, s>>>(F, fr, ce, S2, S1);
  k_stem_bn<<<STEM_C + 32 * B, 256, 0, s>>>(S2, S1, blob, L, (double)B * H * W, momentum, bn, aff1, fold, att, H, W);
  return RGBD_OK;
}

}  // namespace rgbd::rp

#ifdef RGBD_DIAG
extern "C" int rgbd_debug_stem_lag_stamps(void* buf) {
  unsigned long long* p = (unsigned long long*)buf;
  const hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(g_sl_stamps), &p, sizeof(p));
  if (e != hipSuccess) return (int)e;
  sl_stamps_on = p != nullptr;
  return RGBD_OK;
}
#endif
