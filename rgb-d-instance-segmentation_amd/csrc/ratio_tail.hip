// K4 stage file: the tail both precisions share, float32 throughout: the split pools' finish
// (k_rp_pool_finish), conv 256->512 on the 4x4 map + BN + ReLU + GAP (k_rp_tail_convbn) and the
// MLP with its counter-hash dropout (k_rp_tail_fc1, k_rp_tail_head).  Overview: ratio.hip.
#include "ratio_common.hpp"

using namespace rgbd;
using namespace rgbd::rp;

namespace {

// ------------------------------------------------------------------ pool finish
__global__ void k_rp_pool_finish(const float* __restrict__ part, int B, int H, int W, float* __restrict__ pooled) {
  // pooled[b][256][16] = mean over the region = sum of the split partials / count
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= B * C5 * 16) return;
  const int bb = e / (C5 * 16), c = (e / 16) % C5, reg = e % 16;
  const int i = reg / 4, j = reg % 4;
  const int cnt = (((i + 1) * H + 3) / 4 - (i * H) / 4) * (((j + 1) * W + 3) / 4 - (j * W) / 4);
  float s = 0.f;
  for (int sp = 0; sp < POOL_SPLIT; ++sp) s += part[(((long long)bb * 16 + reg) * POOL_SPLIT + sp) * C5 + c];
  pooled[e] = s / (float)cnt;
}

// ------------------------------------------------------------------ tail: conv 256->512 on 4x4
// Tail conv chunks: the 16-channel groups whose partial sums the fused kernel adds in order.
constexpr int TC_C = 16, TC_CHUNKS = C5 / TC_C;

__device__ __forceinline__ float hash_uniform(unsigned long long seed, unsigned long long idx) {
  unsigned long long z = seed + idx * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (float)(z >> 40) * (1.0f / 16777216.0f);
}

// Tail conv 256->512 + BN(512) + ReLU + AdaptiveAvgPool2d(1) in one launch (k_rp_tail_conv +
// k_rp_tail_bn, bitwise the same values): workgroup = two output channels over ALL 256 input
// channels, so the BN of its channels needs no other workgroup.  LDS holds 8 images' pooled maps
// unpadded [256 c][8 b][16] (128 KB: out-of-map taps read 0.f, the padded copy's value) and the
// two channels' filters [256 c][3 ky][2 o][4]; 512 threads, thread = (chunk k, image b, row py): 2 o x
// 4 px of the 16-channel chunk k, accumulated in tail_conv's order
// (cl, ky, kx; mul then add); then z = b6 + the 16 chunk partials in chunk order (tail_bn's
// zval) and tail_bn's statistics / running-stat update / ReLU / mean over the 16 positions, one
// wave per channel.  256 workgroups (one per CU), eight waves each (two per SIMD: the LDS reads of
// one wave under the other's arithmetic).
constexpr int TB_SP = C5 * 8 * 16;                  // floats: pooled, 8 images
constexpr int TB_SW = C5 * 3 * 2 * 4;               // floats: filters of 2 channels
constexpr int TB_ZS = 2 * 32 * 16;                  // floats: z of the 2 channels, B <= 32
constexpr size_t TB_SMEM = (size_t)(TB_SP + TB_SW + TB_ZS) * 4;
static_assert(TB_SMEM <= 163840 && TC_CHUNKS * 2 * 8 * 16 <= TB_SP, "tail conv+bn LDS");
__global__ __launch_bounds__(512) void k_rp_tail_convbn(const float* __restrict__ pooled, int B, int training,
                                                        float momentum, const char* __restrict__ blob, Layout L,
                                                        BnPtrs bn, float* __restrict__ feat) {
  extern __shared__ __attribute__((aligned(16))) float tsm[];
  float* sp = tsm;                  // [256 c][8 b][16]; later the chunk partials [16 k][2 o][8 b][16]
  float* sw = tsm + TB_SP;          // [256 c][3 ky][2 o][4]
  float* zs = sw + TB_SW;           // [2 o][B * 16]
  const int tid = threadIdx.x, o0 = blockIdx.x * 2;
  const float* w6 = (const float*)(blob + L.w6);
  {
    float wv[2 * C5 * 9 / 512];
#pragma unroll
    for (int q = 0; q < 2 * C5 * 9 / 512; ++q) wv[q] = w6[(long long)o0 * C5 * 9 + tid + 512 * q];
#pragma unroll
    for (int q = 0; q < 2 * C5 * 9 / 512; ++q) {
      const int i = tid + 512 * q, ol = i / (C5 * 9), r = i % (C5 * 9), c = r / 9, tap = r % 9;
      sw[((c * 3 + tap / 3) * 2 + ol) * 4 + tap % 3] = wv[q];
    }
  }
  const int ck = tid >> 5, bl = (tid >> 2) & 7, py = tid & 3;
  for (int b0 = 0; b0 < B; b0 += 8) {
    __syncthreads();  // previous group's partial sums consumed
    {
      constexpr int NQ = TB_SP / 4 / 512;  // float4 per thread
      float4 pv[NQ];
#pragma unroll
      for (int u = 0; u < NQ; ++u) {
        const int e = tid + 512 * u, q = e & 3, c = (e >> 2) & (C5 - 1), b = b0 + (e >> 10);
        pv[u] = b < B ? *reinterpret_cast<const float4*>(pooled + ((long long)b * C5 + c) * 16 + 4 * q)
                      : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int u = 0; u < NQ; ++u) {
        const int e = tid + 512 * u, q = e & 3, c = (e >> 2) & (C5 - 1), b = e >> 10;
        *reinterpret_cast<float4*>(sp + (c * 8 + b) * 16 + 4 * q) = pv[u];
      }
    }
    __syncthreads();
    // pixel pairs in two-wide vectors: packed multiplies and adds (v_pk_mul_f32 / v_pk_add_f32),
    // each lane's arithmetic the scalar mul-then-add of tail_conv
    f32x2 acc[2][2];
#pragma unroll
    for (int ol = 0; ol < 2; ++ol)
#pragma unroll
      for (int x = 0; x < 2; ++x) acc[ol][x] = f32x2{0.f, 0.f};
#pragma unroll 4
    for (int cl = 0; cl < TC_C; ++cl) {
      const int c = ck * TC_C + cl;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int y = py + ky - 1;
        float r[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (y >= 0 && y < 4) {
          const float4 v = *reinterpret_cast<const float4*>(sp + (c * 8 + bl) * 16 + 4 * y);
          r[1] = v.x; r[2] = v.y; r[3] = v.z; r[4] = v.w;
        }
        const float4 w0 = *reinterpret_cast<const float4*>(sw + ((c * 3 + ky) * 2 + 0) * 4);
        const float4 w1 = *reinterpret_cast<const float4*>(sw + ((c * 3 + ky) * 2 + 1) * 4);
        const float wa[3] = {w0.x, w0.y, w0.z}, wb[3] = {w1.x, w1.y, w1.z};
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
          for (int x = 0; x < 2; ++x) {
            const f32x2 rv = f32x2{r[2 * x + kx], r[2 * x + 1 + kx]};
            acc[0][x] += f32x2{wa[kx], wa[kx]} * rv;
            acc[1][x] += f32x2{wb[kx], wb[kx]} * rv;
          }
      }
    }
    __syncthreads();  // every thread's pooled reads done: the region takes the chunk partials
#pragma unroll
    for (int ol = 0; ol < 2; ++ol)
      *reinterpret_cast<float4*>(sp + ((ck * 2 + ol) * 8 + bl) * 16 + 4 * py) =
          make_float4(acc[ol][0].x, acc[ol][0].y, acc[ol][1].x, acc[ol][1].y);
    __syncthreads();
    if (tid < 256) {  // z = b6 + the chunk partials in chunk order: thread = (o, image, position)
      const int ol = tid >> 7, b = (tid >> 4) & 7, pos = tid & 15;
      float z = ((const float*)(blob + L.b6))[o0 + ol];
#pragma unroll
      for (int k = 0; k < TC_CHUNKS; ++k) z += sp[((k * 2 + ol) * 8 + b) * 16 + pos];
      if (b0 + b < B) zs[ol * (B * 16) + (b0 + b) * 16 + pos] = z;
    }
  }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  if (wave >= 2) return;
  const int c = o0 + wave, n = B * 16;
  const float* zc = zs + wave * n;
  float mean, var;
  if (training) {
    double s = 0.0, q = 0.0;
    for (int bp = lane; bp < n; bp += 64) {
      const double v = zc[bp];
      s += v;
      q += v * v;
    }
    s = wave_sum_f64(s);
    q = wave_sum_f64(q);
    const double nn = (double)n, m = s / nn;
    double v = q / nn - m * m;
    if (v < 0.0) v = 0.0;
    mean = (float)m;
    var = (float)v;
    if (lane == 0) {
      float* rm = bn.p[5 * 4 + 2];
      float* rv = bn.p[5 * 4 + 3];
      const double unb = nn > 1.0 ? v * nn / (nn - 1.0) : v;
      rm[c] = (1.f - momentum) * rm[c] + momentum * mean;
      rv[c] = (1.f - momentum) * rv[c] + momentum * (float)unb;
    }
  } else {
    mean = bn.p[5 * 4 + 2][c];
    var = bn.p[5 * 4 + 3][c];
  }
  const float sc = bn.p[5 * 4 + 0][c] / sqrtf(var + BN_EPS), sh = bn.p[5 * 4 + 1][c] - mean * sc;
  for (int base = 0; base < n; base += 64) {  // n is a multiple of 16: 16-lane groups are whole images
    const int bp = base + lane;
    float r = bp < n ? fmaxf(zc[bp] * sc + sh, 0.f) : 0.f;
    r += __shfl_xor(r, 8);
    r += __shfl_xor(r, 4);
    r += __shfl_xor(r, 2);
    r += __shfl_xor(r, 1);
    if (bp < n && (lane & 15) == 0) feat[(long long)(bp >> 4) * C6 + c] = r / 16.f;
  }
}

// Linear 512 -> 128 + ReLU + Dropout(0.3): one workgroup per output o, thread = 2 k's for all
// images, fixed-order block reduction per image.
__global__ __launch_bounds__(256) void k_rp_tail_fc1(const float* __restrict__ feat, int B, int training,
                                                     const char* __restrict__ blob, Layout L,
                                                     unsigned long long seed, const unsigned long long* seed_ctr,
                                                     float* __restrict__ h1) {
  __shared__ float red[4][32];
  if (seed_ctr) seed += *seed_ctr;
  const int o = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const float* w7 = (const float*)(blob + L.w7);
  const float wa = w7[o * 512 + t], wb = w7[o * 512 + t + 256];
  // all images' feature loads in flight before the reductions (B <= 32)
  float fa[32], fb[32];
#pragma unroll
  for (int b = 0; b < 32; ++b)
    if (b < B) {
      fa[b] = feat[(long long)b * C6 + t];
      fb[b] = feat[(long long)b * C6 + t + 256];
    }
#pragma unroll
  for (int b = 0; b < 32; ++b)
    if (b < B) {
      float s = wa * fa[b] + wb * fb[b];
      s = wave_sum(s);
      if (lane == 0) red[wv][b] = s;
    }
  __syncthreads();
  if (t < B) {
    const float* b7 = (const float*)(blob + L.b7);
    float s = b7[o] + (((red[0][t] + red[1][t]) + red[2][t]) + red[3][t]);
    s = fmaxf(s, 0.f);
    const int e = t * 128 + o;
    if (training) s = hash_uniform(seed, e) < 0.3f ? 0.f : s / 0.7f;  // Dropout(0.3)
    h1[t * 128 + o] = s;
  }
}

// Linear 128 -> 64 + ReLU + Dropout(0.2), Linear 64 -> 32 + ReLU, Linear 32 -> 1, sigmoid range
// map; one workgroup, the weights row-major in LDS (padded rows: lanes walk output rows).
__global__ __launch_bounds__(512) void k_rp_tail_head(const float* __restrict__ h1g, int B, int training,
                                                      const char* __restrict__ blob, Layout L,
                                                      unsigned long long seed, unsigned long long* seed_ctr,
                                                      float* __restrict__ ratio) {
  // the weights stay row-major in LDS with one float of row padding: the staging writes and the
  // per-output row reads (lanes = outputs, rows 129 / 65 floats apart) are both conflict-free
  // (the transposed images this replaced took 32-way conflicts on every staging write)
  __shared__ float w8s[64][129], w9s[32][65];
  const unsigned long long ctr = seed_ctr ? *seed_ctr : 0ull;
  seed += ctr;
  __shared__ float h1[32][128], h2[32][64], h3[32][32];
  const float* w8 = (const float*)(blob + L.w8);
  const float* b8 = (const float*)(blob + L.b8);
  const float* w9 = (const float*)(blob + L.w9);
  const float* b9 = (const float*)(blob + L.b9);
  const float* w10 = (const float*)(blob + L.w10);
  const float* b10 = (const float*)(blob + L.b10);
  {  // every staging load in flight together, then the LDS writes
    float a8[16], a9[4], ah[8];
#pragma unroll
    for (int q = 0; q < 16; ++q) a8[q] = w8[threadIdx.x + 512 * q];
#pragma unroll
    for (int q = 0; q < 4; ++q) a9[q] = w9[threadIdx.x + 512 * q];
#pragma unroll
    for (int q = 0; q < 8; ++q)
      if (threadIdx.x + 512 * q < B * 128) ah[q] = h1g[threadIdx.x + 512 * q];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int i = threadIdx.x + 512 * q;
      w8s[i / 128][i % 128] = a8[q];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = threadIdx.x + 512 * q;
      w9s[i / 64][i % 64] = a9[q];
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int i = threadIdx.x + 512 * q;
      if (i < B * 128) h1[i / 128][i % 128] = ah[q];
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < B * 64; e += 512) {
    const int bb = e / 64, o = e % 64;
    float s = b8[o];
    for (int k = 0; k < 128; ++k) s += w8s[o][k] * h1[bb][k];
    s = fmaxf(s, 0.f);
    if (training) s = hash_uniform(seed ^ 0x5555ull, e) < 0.2f ? 0.f : s / 0.8f;  // Dropout(0.2)
    h2[bb][o] = s;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < B * 32; e += 512) {
    const int bb = e / 32, o = e % 32;
    float s = b9[o];
    for (int k = 0; k < 64; ++k) s += w9s[o][k] * h2[bb][k];
    h3[bb][o] = fmaxf(s, 0.f);
  }
  __syncthreads();
  // every read of the counter (k_rp_tail_fc1, this kernel's prologue) precedes this store: the
  // next forward (or graph replay) draws fresh dropout masks
  if (training && seed_ctr && threadIdx.x == 0) *seed_ctr = ctr + 1ull;
  if (threadIdx.x < B) {
    const int bb = threadIdx.x;
    float s = b10[0];
    for (int k = 0; k < 32; ++k) s += w10[k] * h3[bb][k];
    ratio[bb] = 0.01f + (0.5f - 0.01f) * (1.f / (1.f + expf(-s)));
  }
}

}  // namespace

namespace rgbd::rp {

int pool_finish(const float* part, int B, int H, int W, float* pooled, hipStream_t s) {
  k_rp_pool_finish<<<ceil_div((long long)B * C5 * 16, 256), 256, 0, s>>>(part, B, H, W, pooled);
  return RGBD_OK;
}

// pooled [B][256][16] -> feat [B][512] -> h1 [B][128] -> ratio [B]
int tail(const float* pooled, int B, int training, float momentum, const char* blob, const Layout& L,
         const BnPtrs& bn, unsigned long long seed, unsigned long long* seed_ctr, float* feat, float* h1, float* ratio,
         hipStream_t s) {
  static const hipError_t tattr =
      hipFuncSetAttribute((const void*)k_rp_tail_convbn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)TB_SMEM);
  if (tattr != hipSuccess) return (int)tattr;
  k_rp_tail_convbn<<<C6 / 2, 512, TB_SMEM, s>>>(pooled, B, training, momentum, blob, L, bn, feat);
  k_rp_tail_fc1<<<128, 256, 0, s>>>(feat, B, training, blob, L, seed, seed_ctr, h1);
  k_rp_tail_head<<<1, 512, 0, s>>>(h1, B, training, blob, L, seed, seed_ctr, ratio);
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

}  // namespace rgbd::rp
