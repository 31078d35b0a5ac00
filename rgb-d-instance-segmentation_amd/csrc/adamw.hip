// The AdamW step of the training loop (the HF Trainer's AdamW, lr 1e-5 constant: finetuning.py:98
// with config.json:12-13), for a list of fp32 parameters with fp32 gradients and moments,
// in one launch: per element the update torch.optim.AdamW (fused) applies —
//   p -= (lr * wd) * p
//   m  = b1 * m + (1 - b1) * g,   v = b2 * v + (1 - b2) * g * g
//   p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// with the step count t read from device memory (a captured graph replays it; the caller adds 1
// before the launch).  HBM-bound: 16 bytes read and 12 written per element (p, g, m, v; p, m, v).
// A workgroup takes 4096 elements of one tensor (16-byte accesses when the tensor allows them);
// the tensor table travels as a kernel argument, so the launch holds no host-side state.
// rgbd_adamw_multi_shadow also writes each updated parameter's bfloat16 copy (round to nearest
// even, the bits torch's .to(bfloat16) gives) into a caller buffer: the bf16 operand the next
// forward's GEMMs read (dense.cast_weight), without a separate cast launch per weight.
//
// Global-norm gradient clipping (the Trainer's max_grad_norm, torch.nn.utils.clip_grad_norm_ as
// called from Trainer._clip_grad_norm behind finetuning.py:98) rides on the same tables:
//   rgbd_grad_sumsq_multi    one double partial per 4096-element chunk of every gradient, in a
//                            workspace slot fixed by (tensor, chunk): no atomics, so the sum does
//                            not depend on workgroup scheduling.  Every square and every addition
//                            is in double (a float32 product is exact in double), from the element
//                            on: the only float32 rounding of the norm is the final cast.
//   rgbd_grad_norm_finalize  one workgroup sums the partials in a fixed order (thread t takes
//                            slots t, t + 256, ...; then the wave and workgroup trees) and writes
//                            {total_norm, min(1, max_norm / (total_norm + 1e-6))} as float32.
//   rgbd_adamw_multi_scaled  the AdamW update on g * *grad_scale (the coefficient above, read
//                            from device memory once per workgroup); the gradients are not written.
//   rgbd_scale_multi         x *= *scale in place, for the stand-alone clip_grad_norm_.
#include "common.hpp"

#include <math.h>

namespace rgbd {
namespace {

constexpr int AW_MAXT = 48;         // tensors per launch (kernel argument table)
constexpr int AW_CHUNK = 4096;      // elements per workgroup
struct AwTable {
  float* p[AW_MAXT];
  const float* g[AW_MAXT];
  float* m[AW_MAXT];
  float* v[AW_MAXT];
  bf16_t* s[AW_MAXT];  // bfloat16 shadow of p (nullptr: none)
  long long n[AW_MAXT];
  int block0[AW_MAXT + 1];  // first workgroup of each tensor
  int nt;
};

struct AwHyper {
  float b1, b2, omb1, omb2;  // beta and 1 - beta (formed in double: 1 - 0.999f is 1.3e-5 off 0.001)
  float lrwd, eps;           // lr * weight_decay
  double b1d, b2d, lr;       // bias corrections in double, per workgroup
};

__device__ __forceinline__ void aw_elem(float& p, float g, float& m, float& v, const AwHyper& h, float step_size,
                                        float bc2_sqrt) {
  p = p - h.lrwd * p;
  m = h.b1 * m + h.omb1 * g;
  v = h.b2 * v + h.omb2 * g * g;
  const float denom = sqrtf(v) / bc2_sqrt + h.eps;
  p = p - step_size * m / denom;
}

// SCALED: every gradient is multiplied by *grad_scale (one float32 rounding, the product torch's
// _foreach_mul_ of the clip coefficient stores) before the update; G itself is only read.
template <bool SCALED>
__global__ __launch_bounds__(256) void k_adamw_multi(const AwTable T, const float* __restrict__ step,
                                                     const AwHyper h, const float* __restrict__ grad_scale) {
  int t = 0;
  for (int i = 1; i < T.nt; ++i)
    if ((int)blockIdx.x >= T.block0[i]) t = i;
  // the bias corrections in double once per workgroup (one lane; double pow is hundreds of
  // instructions), broadcast through LDS
  __shared__ float s_corr[3];
  if (threadIdx.x == 0) {
    if (SCALED) s_corr[2] = *grad_scale;
    const double st = *step;
    const double bc1 = 1.0 - pow(h.b1d, st), bc2 = 1.0 - pow(h.b2d, st);
    s_corr[0] = (float)(h.lr / bc1);
    s_corr[1] = (float)sqrt(bc2);
  }
  __syncthreads();
  const float step_size = s_corr[0], bc2_sqrt = s_corr[1];
  const float gs = SCALED ? s_corr[2] : 1.0f;
  const long long n = T.n[t];
  const long long e0 = (long long)(blockIdx.x - T.block0[t]) * AW_CHUNK;
  float* __restrict__ P = T.p[t];
  const float* __restrict__ G = T.g[t];
  float* __restrict__ M = T.m[t];
  float* __restrict__ V = T.v[t];
  bf16_t* __restrict__ S = T.s[t];
  const bool vec = ((((uintptr_t)P) | ((uintptr_t)G) | ((uintptr_t)M) | ((uintptr_t)V)) & 15) == 0 &&
                   (((uintptr_t)S) & 7) == 0;
  if (vec && e0 + AW_CHUNK <= n) {
#pragma unroll
    for (int k = 0; k < AW_CHUNK / 1024; ++k) {
      const long long e = e0 + 4ll * (threadIdx.x + 256 * k);
      float4 p = *reinterpret_cast<const float4*>(P + e), g = *reinterpret_cast<const float4*>(G + e);
      float4 m = *reinterpret_cast<const float4*>(M + e), v = *reinterpret_cast<const float4*>(V + e);
      if (SCALED) {
        g.x *= gs;
        g.y *= gs;
        g.z *= gs;
        g.w *= gs;
      }
      aw_elem(p.x, g.x, m.x, v.x, h, step_size, bc2_sqrt);
      aw_elem(p.y, g.y, m.y, v.y, h, step_size, bc2_sqrt);
      aw_elem(p.z, g.z, m.z, v.z, h, step_size, bc2_sqrt);
      aw_elem(p.w, g.w, m.w, v.w, h, step_size, bc2_sqrt);
      *reinterpret_cast<float4*>(P + e) = p;
      *reinterpret_cast<float4*>(M + e) = m;
      *reinterpret_cast<float4*>(V + e) = v;
      if (S) *reinterpret_cast<uint2*>(S + e) = make_uint2(pack_bf16x2(p.x, p.y), pack_bf16x2(p.z, p.w));
    }
    return;
  }
  for (long long e = e0 + threadIdx.x; e < e0 + AW_CHUNK && e < n; e += 256) {
    float p = P[e], m = M[e], v = V[e];
    aw_elem(p, SCALED ? G[e] * gs : G[e], m, v, h, step_size, bc2_sqrt);
    P[e] = p;
    M[e] = m;
    V[e] = v;
    if (S) S[e] = f32_to_bf16(p);
  }
}

// ---------------------------------------------------------------- gradient norm and scale
constexpr int MT_MAXT = 128;  // tensors per launch: 20 bytes of kernel argument each (2.6 KB of the 4 KB)
struct MtTable {
  float* x[MT_MAXT];
  long long n[MT_MAXT];
  int block0[MT_MAXT + 1];  // first workgroup of each tensor
  int nt;
};

// the tensor workgroup b works on: the last i with block0[i] <= b (an empty tensor shares its
// block0 with its successor and is never chosen)
#define RGBD_MT_TENSOR(T, b, t)              \
  int t = 0;                                 \
  for (int hi__ = (T).nt - 1; t < hi__;) {   \
    const int mid__ = (t + hi__ + 1) >> 1;   \
    if ((T).block0[mid__] <= (b))            \
      t = mid__;                             \
    else                                     \
      hi__ = mid__ - 1;                      \
  }

// the workgroup's 256 values summed in a fixed tree (xor butterflies within a wave, then the four
// wave sums in wave order); the result is valid in thread 0
__device__ __forceinline__ double block_sum_f64(double v) {
  __shared__ double s_w[4];
  v = wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

// Thread t owns elements 4 * (t + 256 k) .. + 3, k = 0..3, of the chunk on both paths, so the
// summation order (and with it every bit of the partial) does not depend on the pointer's
// alignment; the 16-byte path only loads them with one instruction each.
__global__ __launch_bounds__(256) void k_grad_sumsq(const MtTable T, double* __restrict__ partials) {
  RGBD_MT_TENSOR(T, (int)blockIdx.x, t)
  const long long n = T.n[t];
  const long long e0 = (long long)(blockIdx.x - T.block0[t]) * AW_CHUNK;
  const float* __restrict__ G = T.x[t];
  double acc = 0.0;
  if ((((uintptr_t)G) & 15) == 0 && e0 + AW_CHUNK <= n) {
    float4 g[AW_CHUNK / 1024];
#pragma unroll
    for (int k = 0; k < AW_CHUNK / 1024; ++k)
      g[k] = *reinterpret_cast<const float4*>(G + e0 + 4ll * (threadIdx.x + 256 * k));
#pragma unroll
    for (int k = 0; k < AW_CHUNK / 1024; ++k) {
      acc += (double)g[k].x * (double)g[k].x;
      acc += (double)g[k].y * (double)g[k].y;
      acc += (double)g[k].z * (double)g[k].z;
      acc += (double)g[k].w * (double)g[k].w;
    }
  } else {
    for (int k = 0; k < AW_CHUNK / 1024; ++k) {
      const long long e = e0 + 4ll * (threadIdx.x + 256 * k);
      for (int j = 0; j < 4; ++j)
        if (e + j < n) {
          const double d = G[e + j];
          acc += d * d;
        }
    }
  }
  acc = block_sum_f64(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

__global__ __launch_bounds__(256) void k_grad_norm_finalize(const double* __restrict__ partials, long long n,
                                                            float max_norm, float* __restrict__ out) {
  double acc = 0.0;
  for (long long i = threadIdx.x; i < n; i += 256) acc += partials[i];
  acc = block_sum_f64(acc);
  if (threadIdx.x == 0) {
    // torch.nn.utils.clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6) — a float32
    // tensor's __rtruediv__, i.e. reciprocal() * max_norm — then clamp(max=1.0).  NaN stays NaN
    // (the comparison is false), an infinite norm gives 0.
    const float norm = (float)sqrt(acc);
    float coef = (1.0f / (norm + 1e-6f)) * max_norm;
    coef = coef > 1.0f ? 1.0f : coef;
    out[0] = norm;
    out[1] = coef;
  }
}

__global__ __launch_bounds__(256) void k_scale_multi(const MtTable T, const float* __restrict__ scale) {
  RGBD_MT_TENSOR(T, (int)blockIdx.x, t)
  const float s = *scale;
  const long long n = T.n[t];
  const long long e0 = (long long)(blockIdx.x - T.block0[t]) * AW_CHUNK;
  float* __restrict__ X = T.x[t];
  if ((((uintptr_t)X) & 15) == 0 && e0 + AW_CHUNK <= n) {
#pragma unroll
    for (int k = 0; k < AW_CHUNK / 1024; ++k) {
      const long long e = e0 + 4ll * (threadIdx.x + 256 * k);
      float4 x = *reinterpret_cast<const float4*>(X + e);
      x.x *= s;
      x.y *= s;
      x.z *= s;
      x.w *= s;
      *reinterpret_cast<float4*>(X + e) = x;
    }
    return;
  }
  for (long long e = e0 + threadIdx.x; e < e0 + AW_CHUNK && e < n; e += 256) X[e] *= s;
}

}  // namespace
}  // namespace rgbd

using namespace rgbd;

static int adamw_launch(int n, float* const* params, const float* const* grads, float* const* exp_avg,
                        float* const* exp_avg_sq, void* const* shadows, const long long* numel, const float* step,
                        const float* grad_scale, double lr, double beta1, double beta2, double eps,
                        double weight_decay, void* stream) {
  RGBD_REQUIRE(n >= 1 && n <= AW_MAXT && params && grads && exp_avg && exp_avg_sq && numel && step, RGBD_E_ARG);
  AwTable T;
  long long blocks = 0;
  for (int i = 0; i < n; ++i) {
    RGBD_REQUIRE(numel[i] >= 0, RGBD_E_ARG);
    RGBD_REQUIRE(numel[i] == 0 || (params[i] && grads[i] && exp_avg[i] && exp_avg_sq[i]), RGBD_E_ARG);
    T.p[i] = params[i];
    T.g[i] = grads[i];
    T.m[i] = exp_avg[i];
    T.v[i] = exp_avg_sq[i];
    T.s[i] = shadows ? (bf16_t*)shadows[i] : nullptr;
    T.n[i] = numel[i];
    T.block0[i] = (int)blocks;
    blocks += (numel[i] + AW_CHUNK - 1) / AW_CHUNK;
  }
  RGBD_REQUIRE(blocks < (1ll << 31), RGBD_E_SHAPE);
  T.block0[n] = (int)blocks;
  T.nt = n;
  if (blocks == 0) return RGBD_OK;
  AwHyper h;
  h.b1 = (float)beta1;
  h.b2 = (float)beta2;
  h.omb1 = (float)(1.0 - beta1);
  h.omb2 = (float)(1.0 - beta2);
  h.lrwd = (float)lr * (float)weight_decay;
  h.eps = (float)eps;
  h.b1d = beta1;
  h.b2d = beta2;
  h.lr = lr;
  if (grad_scale)
    k_adamw_multi<true><<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(T, step, h, grad_scale);
  else
    k_adamw_multi<false><<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(T, step, h, nullptr);
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

// the table of one norm / scale launch from the host arrays; a status on a bad entry
static int mt_table(MtTable& T, int n, float* const* x, const long long* numel) {
  long long blocks = 0;
  for (int i = 0; i < n; ++i) {
    RGBD_REQUIRE(numel[i] >= 0 && (numel[i] == 0 || x[i]), RGBD_E_ARG);
    T.x[i] = x[i];
    T.n[i] = numel[i];
    T.block0[i] = (int)blocks;
    blocks += (numel[i] + AW_CHUNK - 1) / AW_CHUNK;
    RGBD_REQUIRE(blocks < (1ll << 31), RGBD_E_SHAPE);
  }
  T.block0[n] = (int)blocks;
  T.nt = n;
  return RGBD_OK;
}

extern "C" {

int rgbd_adamw_multi(int n, float* const* params, const float* const* grads, float* const* exp_avg,
                     float* const* exp_avg_sq, const long long* numel, const float* step, double lr, double beta1,
                     double beta2, double eps, double weight_decay, void* stream) {
  return adamw_launch(n, params, grads, exp_avg, exp_avg_sq, nullptr, numel, step, nullptr, lr, beta1, beta2, eps,
                      weight_decay, stream);
}

int rgbd_adamw_multi_shadow(int n, float* const* params, const float* const* grads, float* const* exp_avg,
                            float* const* exp_avg_sq, void* const* shadows, const long long* numel, const float* step,
                            double lr, double beta1, double beta2, double eps, double weight_decay, void* stream) {
  RGBD_REQUIRE(shadows, RGBD_E_ARG);
  return adamw_launch(n, params, grads, exp_avg, exp_avg_sq, shadows, numel, step, nullptr, lr, beta1, beta2, eps,
                      weight_decay, stream);
}

int rgbd_adamw_multi_scaled(int n, float* const* params, const float* const* grads, float* const* exp_avg,
                            float* const* exp_avg_sq, void* const* shadows, const long long* numel,
                            const float* step, const float* grad_scale, double lr, double beta1, double beta2,
                            double eps, double weight_decay, void* stream) {
  RGBD_REQUIRE(n >= 0, RGBD_E_ARG);
  if (n == 0) return RGBD_OK;
  RGBD_REQUIRE(grad_scale, RGBD_E_ARG);
  return adamw_launch(n, params, grads, exp_avg, exp_avg_sq, shadows, numel, step, grad_scale, lr, beta1, beta2,
                      eps, weight_decay, stream);
}

size_t rgbd_grad_sumsq_workspace_size(int n, const long long* numel) {
  if (n <= 0 || !numel) return 0;
  size_t slots = 0;
  for (int i = 0; i < n; ++i)
    if (numel[i] > 0) slots += (size_t)((numel[i] + AW_CHUNK - 1) / AW_CHUNK);
  return slots * sizeof(double);
}

int rgbd_grad_sumsq_multi(int n, const float* const* grads, const long long* numel, void* ws, long long slot0,
                          void* stream) {
  RGBD_REQUIRE(n >= 0 && slot0 >= 0, RGBD_E_ARG);
  if (n == 0) return RGBD_OK;
  RGBD_REQUIRE(n <= MT_MAXT && grads && numel && ws, RGBD_E_ARG);
  MtTable T;
  if (int rc = mt_table(T, n, (float* const*)grads, numel)) return rc;
  if (T.block0[n] == 0) return RGBD_OK;
  k_grad_sumsq<<<(unsigned)T.block0[n], 256, 0, (hipStream_t)stream>>>(T, (double*)ws + slot0);
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

int rgbd_grad_norm_finalize(const void* ws, long long n_partials, double max_norm, float* out, void* stream) {
  RGBD_REQUIRE(n_partials >= 0 && (n_partials == 0 || ws), RGBD_E_ARG);
  if (!out) {  // nothing to write: only the empty call may omit it
    RGBD_REQUIRE(n_partials == 0, RGBD_E_ARG);
    return RGBD_OK;
  }
  k_grad_norm_finalize<<<1, 256, 0, (hipStream_t)stream>>>((const double*)ws, n_partials, (float)max_norm, out);
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

int rgbd_scale_multi(int n, float* const* tensors, const long long* numel, const float* scale, void* stream) {
  RGBD_REQUIRE(n >= 0, RGBD_E_ARG);
  if (n == 0) return RGBD_OK;
  RGBD_REQUIRE(n <= MT_MAXT && tensors && numel && scale, RGBD_E_ARG);
  MtTable T;
  if (int rc = mt_table(T, n, tensors, numel)) return rc;
  if (T.block0[n] == 0) return RGBD_OK;
  k_scale_multi<<<(unsigned)T.block0[n], 256, 0, (hipStream_t)stream>>>(T, scale);
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

}  // extern "C"
