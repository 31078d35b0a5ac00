// f3: the classification term of the Mask2Former loss — weighted cross-entropy over every
// (image, query) row, with the targets built from the batched assignment (gfx950).
//
// Reference (third-party, called by the model the reference trains): transformers 5.15
// modeling_mask2former.py Mask2FormerLoss.loss_labels :548-578 — the matched queries get their
// target's class, every other query "no object" (the last class), then
// nn.CrossEntropyLoss(weight=empty_weight): sum_i w[t_i] (lse_i - x[i][t_i]) / sum_i w[t_i].
//
//   k_class_loss_fwd    one workgroup per CL_ROWS consecutive rows.  The rows' logits are staged
//                       into LDS as float32 with 16-byte loads over the FLAT [N C1] array (a row
//                       of an odd C1 is not 16-byte aligned, a block of 8 rows is), the block's
//                       targets are built in LDS from the matches of the images it overlaps, then
//                       a group of G lanes reduces each row (G = 16: four rows per wave, up to
//                       C1 = 64; G = 64: a wave per row above that): max, sum exp(x - max), the
//                       row's w[t] (log s - (x[t] - max)).  Thread 0 adds the block's rows in row
//                       order into one (numerator, denominator) pair of the workspace.
//   k_class_loss_final  one workgroup: the pairs added in a fixed strided + tree order, the
//                       division, and the weight sum kept for the backward.
//   k_class_loss_bwd    elementwise over the flat array, four elements per thread:
//                       g w[t]/W (exp((x - max) - log s) - [c == t]), stored in the logits' dtype.
//
// No float atomics; every sum's order is a function of (B, Q, C1) alone.  The row statistics are
// kept as (max, log s) and not as their sum: at logits of 1e4 the sum's float32 spacing (2^-8)
// would be the relative error of every probability the backward rebuilds.
#include <cmath>

#include "common.hpp"

using namespace rgbd;

namespace {

constexpr int CL_THR = 256;
constexpr int CL_ROWS = 16;          // rows per workgroup: a multiple of 8, so the block's flat
                                     // range starts 16-byte aligned for float32 and bfloat16
constexpr int CL_MAX_C1 = 512;       // CL_ROWS rows of float32 in LDS: 32 KiB
constexpr int CL_FINAL_THR = 256;

template <typename T> struct Vec;
template <> struct Vec<float> {
  static constexpr int N = 4;
  typedef f32x4 type;
};
template <> struct Vec<bf16_t> {
  static constexpr int N = 8;
  typedef u16x8 type;
};

inline int cl_blocks(long long N) { return (int)((N + CL_ROWS - 1) / CL_ROWS); }
inline size_t cl_smem(int C1) { return ((size_t)CL_ROWS * C1 + 3 * CL_ROWS) * 4; }

template <int G>
__device__ __forceinline__ float group_max(float v) {
  for (int o = G / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
template <int G>
__device__ __forceinline__ float group_sum(float v) {
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <typename T, int G>
__global__ __launch_bounds__(CL_THR) void k_class_loss_fwd(
    const T* __restrict__ x, const float* __restrict__ w, int N, int Q, int C1, const long long* __restrict__ rows_all,
    const long long* __restrict__ cols_all, int M, const int* __restrict__ moff, const int* __restrict__ toff,
    const long long* __restrict__ labels, int Tn, int vec_ok, float* __restrict__ partial, float* __restrict__ stats,
    int* __restrict__ target) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* tile = reinterpret_cast<float*>(smem);  // [CL_ROWS][C1]
  int* tg = reinterpret_cast<int*>(tile + CL_ROWS * C1);
  float* rnum = reinterpret_cast<float*>(tg + CL_ROWS);
  float* rden = rnum + CL_ROWS;
  const int tid = threadIdx.x;
  const int r0 = blockIdx.x * CL_ROWS;
  const int nrows = min(CL_ROWS, N - r0);
  const int ne = nrows * C1;
  const T* src = x + (long long)r0 * C1;

  // the block's logits, flat, widened to float32
  constexpr int VN = Vec<T>::N;
  const int nv = vec_ok ? ne / VN : 0;
  for (int v = tid; v < nv; v += CL_THR) {
    const typename Vec<T>::type q = reinterpret_cast<const typename Vec<T>::type*>(src)[v];
#pragma unroll
    for (int k = 0; k < VN; k += 4) {
      f32x4 o;
      o[0] = Num<T>::to_f(q[k]);
      o[1] = Num<T>::to_f(q[k + 1]);
      o[2] = Num<T>::to_f(q[k + 2]);
      o[3] = Num<T>::to_f(q[k + 3]);
      *reinterpret_cast<f32x4*>(tile + v * VN + k) = o;
    }
  }
  for (int e = nv * VN + tid; e < ne; e += CL_THR) tile[e] = Num<T>::to_f(src[e]);

  // the block's targets: no object, then the matches of the images these rows belong to.  An
  // index outside its range (query, target, class) leaves the row at no object: nothing is read
  // or written out of bounds for any contents of the index arrays.
  if (tid < CL_ROWS) tg[tid] = C1 - 1;
  __syncthreads();
  const int b0 = r0 / Q, b1 = (r0 + nrows - 1) / Q;
  const int ms = max(moff[b0], 0), me = min(moff[b1 + 1], M);
  for (int m = ms + tid; m < me; m += CL_THR) {
    int b = b0;
    while (b < b1 && m >= moff[b + 1]) ++b;
    const long long q = rows_all[m], col = cols_all[m];
    if (q < 0 || q >= Q || col < 0) continue;
    const long long row = (long long)b * Q + q - r0;
    const long long li = (long long)toff[b] + col;
    if (row < 0 || row >= nrows || li < 0 || li >= toff[b + 1] || li >= Tn) continue;
    const long long lab = labels[li];
    if (lab < 0 || lab >= C1) continue;
    tg[row] = (int)lab;
  }
  __syncthreads();

  // one group of G lanes per row; a group past the block's last row computes row 0 and drops it
  const int grp = tid / G, lane = tid % G;
  for (int r = grp; r < CL_ROWS; r += CL_THR / G) {
    const bool live = r < nrows;
    const float* xr = tile + (live ? r : 0) * C1;
    float mx = -INFINITY;
    for (int c = lane; c < C1; c += G) mx = fmaxf(mx, xr[c]);
    mx = group_max<G>(mx);
    float s = 0.f;
    for (int c = lane; c < C1; c += G) s += expf(xr[c] - mx);  // exp(-inf) = 0
    s = group_sum<G>(s);
    if (lane == 0) {
      float num = 0.f, den = 0.f;
      if (live) {
        const int t = tg[r];
        const float ls = logf(s);
        den = w[t];
        num = den * (ls - (xr[t] - mx));
        stats[r0 + r] = mx;
        stats[(long long)N + r0 + r] = ls;
        target[r0 + r] = t;
      }
      rnum[r] = num;
      rden[r] = den;
    }
  }
  __syncthreads();
  if (tid == 0) {
    float num = 0.f, den = 0.f;
    for (int r = 0; r < CL_ROWS; ++r) {
      num += rnum[r];
      den += rden[r];
    }
    partial[2 * blockIdx.x] = num;
    partial[2 * blockIdx.x + 1] = den;
  }
}

// *loss = sum num / sum den over the nblk block pairs, *wsum = sum den.  The
// denominator is not guarded (an all-zero weight sum gives NaN, as torch does).
__global__ __launch_bounds__(CL_FINAL_THR) void k_class_loss_final(const float* __restrict__ partial, int nblk,
                                                                 float* __restrict__ loss, float* __restrict__ wsum) {
  __shared__ float sn[CL_FINAL_THR], sd[CL_FINAL_THR];
  const int tid = threadIdx.x;
  float num = 0.f, den = 0.f;
  for (int i = tid; i < nblk; i += CL_FINAL_THR) {
    num += partial[2 * i];
    den += partial[2 * i + 1];
  }
  sn[tid] = num;
  sd[tid] = den;
  __syncthreads();
  for (int o = CL_FINAL_THR / 2; o > 0; o >>= 1) {
    if (tid < o) {
      sn[tid] += sn[tid + o];
      sd[tid] += sd[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    *loss = sn[0] / sd[0];
    *wsum = sd[0];
  }
}

template <typename T>
__global__ __launch_bounds__(CL_THR) void k_class_loss_bwd(const T* __restrict__ x, const float* __restrict__ w, int N,
                                                         int C1, const float* __restrict__ stats,
                                                         const int* __restrict__ target, const float* __restrict__ wsum,
                                                         const float* __restrict__ g, int vec_ok, T* __restrict__ gx) {
  const long long total = (long long)N * C1;
  const long long i0 = (blockIdx.x * (long long)CL_THR + threadIdx.x) * 4;
  if (i0 >= total) return;
  const float scale = *g / *wsum;
  const int n = (int)min(4ll, total - i0);
  float xv[4], gv[4];
  const bool wide = vec_ok && n == 4;
  if (wide) {
    if constexpr (sizeof(T) == 4) {
      const f32x4 q = *reinterpret_cast<const f32x4*>(x + i0);
      for (int e = 0; e < 4; ++e) xv[e] = q[e];
    } else {
      const u16x4 q = *reinterpret_cast<const u16x4*>(x + i0);
      for (int e = 0; e < 4; ++e) xv[e] = bf16_to_f32(q[e]);
    }
  } else {
    for (int e = 0; e < n; ++e) xv[e] = Num<T>::to_f(x[i0 + e]);
  }
  for (int e = 0; e < n; ++e) {
    const int row = (int)((i0 + e) / C1), c = (int)((i0 + e) - (long long)row * C1);
    const int t = target[row];
    const float coef = (unsigned)t < (unsigned)C1 ? w[t] * scale : 0.f;
    const float p = expf((xv[e] - stats[row]) - stats[(long long)N + row]);
    gv[e] = coef * (p - (c == t ? 1.f : 0.f));
  }
  if (wide) {
    if constexpr (sizeof(T) == 4) {
      f32x4 q;
      for (int e = 0; e < 4; ++e) q[e] = gv[e];
      *reinterpret_cast<f32x4*>(gx + i0) = q;
    } else {
      u16x4 q;
      for (int e = 0; e < 4; ++e) q[e] = f32_to_bf16(gv[e]);  // the one rounding
      *reinterpret_cast<u16x4*>(gx + i0) = q;
    }
  } else {
    for (int e = 0; e < n; ++e) gx[i0 + e] = Num<T>::from_f(gv[e]);
  }
}

// the checks both entry points share; everything here runs before any HIP call
int cl_check(int dtype, int B, int Q, int C1) {
  RGBD_REQUIRE(B > 0 && Q > 0 && C1 > 0, RGBD_E_ARG);
  RGBD_REQUIRE(dtype == RGBD_F32 || dtype == RGBD_BF16, RGBD_E_DTYPE);
  RGBD_REQUIRE(C1 >= 2 && C1 <= CL_MAX_C1 && (long long)B * Q * C1 < (1ll << 31), RGBD_E_SHAPE);
  return RGBD_OK;
}

template <typename T>
void cl_launch_fwd(const void* logits, const float* w, int N, int Q, int C1, const long long* rows_all,
                  const long long* cols_all, int M, const int* moff, const int* toff, const long long* labels, int Tn,
                  float* partial, float* stats, int* target, hipStream_t s) {
  const int vec_ok = ((uintptr_t)logits & 15) == 0;
  auto* kern = C1 <= 64 ? k_class_loss_fwd<T, 16> : k_class_loss_fwd<T, 64>;
  kern<<<cl_blocks(N), CL_THR, cl_smem(C1), s>>>((const T*)logits, w, N, Q, C1, rows_all, cols_all, M, moff, toff, labels,
                                                 Tn, vec_ok, partial, stats, target);
}

}  // namespace

extern "C" {

int rgbd_class_loss_max_classes() { return CL_MAX_C1; }

size_t rgbd_class_loss_workspace_size(int B, int Q, int C1) {
  if (B <= 0 || Q <= 0 || C1 <= 0) return 0;
  return align256((size_t)cl_blocks((long long)B * Q) * 2 * sizeof(float));
}

int rgbd_class_loss_fwd(int dtype, const void* logits, const float* w, int B, int Q, int C1,
                        const long long* rows_all, const long long* cols_all, int M, const int* moff, const int* toff,
                        const long long* labels_all, int T, void* ws, float* loss, float* wsum, float* stats,
                        int* target, void* stream) {
  RGBD_REQUIRE(logits && w && moff && toff && ws && loss && wsum && stats && target && M >= 0 && T >= 0, RGBD_E_ARG);
  RGBD_REQUIRE(M == 0 || (rows_all && cols_all && labels_all), RGBD_E_ARG);
  const int rc = cl_check(dtype, B, Q, C1);
  if (rc != RGBD_OK) return rc;
  const int N = B * Q;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == RGBD_F32)
    cl_launch_fwd<float>(logits, w, N, Q, C1, rows_all, cols_all, M, moff, toff, labels_all, T, (float*)ws, stats,
                         target, s);
  else
    cl_launch_fwd<bf16_t>(logits, w, N, Q, C1, rows_all, cols_all, M, moff, toff, labels_all, T, (float*)ws, stats,
                          target, s);
  RGBD_CHECK_LAUNCH();
  k_class_loss_final<<<1, CL_FINAL_THR, 0, s>>>((const float*)ws, cl_blocks(N), loss, wsum);
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

int rgbd_class_loss_bwd(int dtype, const void* logits, const float* w, int B, int Q, int C1, const float* stats,
                        const int* target, const float* wsum, const float* g, void* glogits, void* stream) {
  RGBD_REQUIRE(logits && w && stats && target && wsum && g && glogits, RGBD_E_ARG);
  const int rc = cl_check(dtype, B, Q, C1);
  if (rc != RGBD_OK) return rc;
  const int N = B * Q;
  const long long total = (long long)N * C1;
  const unsigned grid = (unsigned)((total + 4ll * CL_THR - 1) / (4ll * CL_THR));
  const int vec_ok = (((uintptr_t)logits | (uintptr_t)glogits) & 15) == 0;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == RGBD_F32)
    k_class_loss_bwd<float><<<grid, CL_THR, 0, s>>>((const float*)logits, w, N, C1, stats, target, wsum, g, vec_ok,
                                                   (float*)glogits);
  else
    k_class_loss_bwd<bf16_t><<<grid, CL_THR, 0, s>>>((const bf16_t*)logits, w, N, C1, stats, target, wsum, g, vec_ok,
                                                    (bf16_t*)glogits);
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

}  // extern "C"
