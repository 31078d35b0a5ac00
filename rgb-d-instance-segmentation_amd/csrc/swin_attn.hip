// f2: Swin-T's (shifted-)window multi-head self-attention on gfx950, the core of
// every SwinLayer of the backbone the reference calls at custom_model.py:330
// (transformers 5.15 modeling_swin.py SwinLayer.forward :529-582, SwinAttention.forward
// :418-468, eager_attention_forward :373-398, get_attn_mask :591-610).
//
// HF pads the LayerNorm'ed map to multiples of the window (zeros), rolls it by -shift, cuts
// 7x7 windows, projects q/k/v, adds the relative-position bias (table[(2w-1)^2][heads] gathered
// by a fixed index) and the shift mask (-100 between tokens of different shift regions),
// softmax, P.V, and undoes window / roll / pad.  Projections are per token, so here q/k/v are
// projected on the ORIGINAL token layout (one GEMM) and this kernel does the rest by index
// arithmetic: a window token (i, j) of window (wy, wx) in the rolled padded map is padded-map
// position ((7wy + i + s) mod Hp, (7wx + j + s) mod Wp); inside the H x W map it is that token's
// projection, outside it is a zero row's projection, i.e. the projection biases.  The output
// goes straight back to the token's original row.
//
// One wave per (image, window, head), head_dim 32, the 49 tokens padded to 64:
//   S^T = K Q^T   (MFMA: A = key rows, B = query rows; q and k fragments loaded straight from
//                 global, 8 consecutive dims per lane = one K step of 32 = head_dim)
//   s = S * scale + bias[h][idx(q, k)] + shift mask, keys >= 49 excluded; softmax per query
//   column in float32 (keys sit on the lane's 4 registers, its lane group and the 4 key tiles)
//   O^T = V^T P^T (MFMA: A = V^T from a transposed LDS copy of V, B = P^T straight from the
//                 accumulators — the k order of each 32-key step is the accumulators' own,
//                 applied to both operands), normalised by the row sum, 4 consecutive dims per
//                 lane stored to the query token's row.
// bf16: v_mfma_f32_16x16x32_bf16 (P rounded to bf16 as HF's eager path rounds it); f32: exact
// f32 MFMA.  Bound: latency / L2 (per (window, head) 64 x 32 x 3 operands, 2 x 49^2 x 32 MACs).
#include "common.hpp"
#include "mfma.hpp"

namespace rgbd {
namespace {

constexpr int SW_WS = 7, SW_T = 49, SW_HD = 32;
constexpr int SW_TABLE = (2 * SW_WS - 1) * (2 * SW_WS - 1);  // 169
constexpr int SW_WAVES = 4;

struct SwinArgs {
  const void *q, *k, *v;
  long long ldq;  // row stride (elements) of q / k / v (3C when they share one GEMM output)
  const float *bq, *bk, *bv;  // projection biases (padded-map tokens), may be NULL
  const float* table;         // [169][heads]
  void* out;                  // [B*H*W][ldo]
  long long ldo;
  int B, H, W, heads, shift, Hp, Wp, nwy, nwx;
  float scale;
};

template <typename T> struct SwT;
template <> struct SwT<bf16_t> {
  static constexpr int VT_S = 64 + 8;  // Vt row (keys) stride, bf16 elements
};
template <> struct SwT<float> {
  static constexpr int VT_S = 64 + 4;
};

__device__ __forceinline__ int sw_region(int y, int Hp, int s) { return (y >= Hp - SW_WS) + (y >= Hp - s); }

template <typename T>
__global__ __launch_bounds__(64 * SW_WAVES) void k_swin_attn(SwinArgs a) {
  __shared__ __attribute__((aligned(16))) T vts[SW_WAVES][SW_HD][SwT<T>::VT_S];
  __shared__ float tab[SW_WAVES][SW_TABLE + 3];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long item = (long long)blockIdx.x * SW_WAVES + wv;
  const long long total = (long long)a.B * a.nwy * a.nwx * a.heads;
  if (item >= total) return;  // wave-uniform; no workgroup barrier below
  const int h = (int)(item % a.heads);
  long long rest = item / a.heads;
  const int wx = (int)(rest % a.nwx);
  rest /= a.nwx;
  const int wy = (int)(rest % a.nwy);
  const int b = (int)(rest / a.nwy);
  const int r = lane & 15, g = lane >> 4;
  T* vt = &vts[wv][0][0];
  float* tb = tab[wv];
  for (int i = lane; i < SW_TABLE; i += 64) tb[i] = a.table[i * a.heads + h];

  // token t of the window -> original row (or -1: padded-map position, projection = bias)
  auto token_row = [&](int t, int* region) -> long long {
    const int ti = t / SW_WS, tj = t % SW_WS;
    const int ys = wy * SW_WS + ti, xs = wx * SW_WS + tj;  // rolled padded map
    if (region) *region = a.shift > 0 ? 3 * sw_region(ys, a.Hp, a.shift) + sw_region(xs, a.Wp, a.shift) : 0;
    const int py = a.shift > 0 ? (ys + a.shift) % a.Hp : ys, px = a.shift > 0 ? (xs + a.shift) % a.Wp : xs;
    if (py >= a.H || px >= a.W) return -1;
    return ((long long)b * a.H + py) * a.W + px;
  };
  // 8 consecutive head dims (8g..8g+7) of token t's q / k / v row
  // The row's load is unconditional (a clamped row) and only the rare lanes of padded tokens
  // overwrite it: with the load inside an if / else the compiler waited for it at the join, so
  // every call was a memory round trip.
  auto frag_of = [&](const void* base, const float* bias, int t) -> Frag<T> {
    Frag<T> f;
    const long long row = t < SW_T ? token_row(t, nullptr) : -1;
    const int d0 = h * SW_HD + 8 * g;
    f.load(reinterpret_cast<const T*>(base) + (row >= 0 ? row : 0) * a.ldq + d0);
    if (row < 0) {
      if (t >= SW_T) {
        f.zero();
      } else {
        float e[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] = bias ? bias[d0 + j] : 0.f;
        f.from8(e);  // the GEMM output of a zero row: bias (rounded to the operand dtype)
      }
    }
    return f;
  };

  // V^T into LDS: lane = token, its 32 dims as four 8-dim fragments
  {
    const int t = lane;
    // the row's four fragments loaded first and unconditionally (a clamped row), then converted;
    // only the rare lanes of padded tokens overwrite them with the bias (as frag_of): inside an
    // if / else, or converted as they arrive, each load was a memory round trip of its own
    const long long row = t < SW_T ? token_row(t, nullptr) : -1;
    Frag<T> fv[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) fv[c].load(reinterpret_cast<const T*>(a.v) + (row >= 0 ? row : 0) * a.ldq + h * SW_HD + 8 * c);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int d0 = h * SW_HD + 8 * c;
      float e[8];
      fv[c].to8(e);
      if (row < 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          e[j] = t < SW_T && a.bv ? Num<T>::to_f(Num<T>::from_f(a.bv[d0 + j])) : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) vt[(8 * c + j) * SwT<T>::VT_S + t] = Num<T>::from_f(e[j]);
    }
  }
  Frag<T> kf[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) kf[j] = frag_of(a.k, a.bk, 16 * j + r);
  __builtin_amdgcn_wave_barrier();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

  for (int qi = 0; qi < 4; ++qi) {
    const int tq = 16 * qi + r;  // this lane's query (column of S^T)
    int qreg = 0;
    const long long qrow = tq < SW_T ? token_row(tq, &qreg) : -1;
    const Frag<T> qf = frag_of(a.q, a.bq, tq);
    const int qy = tq / SW_WS, qx = tq % SW_WS;
    f32x4 s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      mma(s[j], kf[j], qf);
    }
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int tk = 16 * j + 4 * g + e;
        float v = -INFINITY;
        if (tk < SW_T) {
          const int ky = tk / SW_WS, kx = tk % SW_WS;
          const int idx = (qy - ky + SW_WS - 1) * (2 * SW_WS - 1) + (qx - kx + SW_WS - 1);
          int kreg = 0;
          if (a.shift > 0) token_row(tk, &kreg);
          // HF: (q k^T) * scale + (bias + shift mask), the mask added to the bias first
          const float bm = tb[idx] + (a.shift > 0 && kreg != qreg ? -100.f : 0.f);
          v = s[j][e] * a.scale + bm;
        }
        s[j][e] = v;
        mx = fmaxf(mx, v);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float l = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float p = s[j][e] == -INFINITY ? 0.f : expf(s[j][e] - mx);
        s[j][e] = p;
        l += p;
      }
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    const float inv = 1.f / l;
    // P^T as the B operand: 32-key step kp covers key tiles 2kp, 2kp+1; element e of the first
    // half is key 16(2kp) + 4g + e, of the second half key 16(2kp+1) + 4g + e.  The softmax is
    // normalised before the rounding to the operand dtype, as HF's softmax(...).to(dtype).
    Frag<T> pf[2];
#pragma unroll
    for (int kp = 0; kp < 2; ++kp) {
      float e8[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        e8[e] = s[2 * kp][e] * inv;
        e8[4 + e] = s[2 * kp + 1][e] * inv;
      }
      pf[kp].from8(e8);
    }
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kp = 0; kp < 2; ++kp) {
        // V^T fragment in the same key order: dims 16 dt + r, keys 16(2kp) + 4g + 0..3 and
        // 16(2kp+1) + 4g + 0..3
        const T* row = vt + (16 * dt + r) * SwT<T>::VT_S;
        float e8[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          e8[e] = Num<T>::to_f(row[32 * kp + 4 * g + e]);
          e8[4 + e] = Num<T>::to_f(row[32 * kp + 16 + 4 * g + e]);
        }
        Frag<T> vf;
        vf.from8(e8);
        mma(o, vf, pf[kp]);
      }
      // o[e] = O^T[dim 16 dt + 4 g + e][query tq]
      if (qrow >= 0) {
        T* dst = reinterpret_cast<T*>(a.out) + qrow * a.ldo + h * SW_HD + 16 * dt + 4 * g;
        if constexpr (sizeof(T) == 2) {
          *reinterpret_cast<uint2*>(dst) = make_uint2(pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]));
        } else {
          *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------- backward
// One wave per (image, window, head) again.  Nothing of the forward is stored: S and P are
// recomputed with the forward's index arithmetic, mask and exclusions, once per orientation,
// because the accumulators of a 16x16 tile serve as the B operand of the next product only
// along the dimension that sits on their registers:
//   pass 1, per query tile (lane r = query, registers = keys; the forward's orientation):
//     S^T = K Q^T, P^T, dP^T = V dO^T (rounded to the operand dtype as a GEMM output),
//     D_q = sum_k P dP (= sum_d dO O with O = P V recomputed and contracted in the other order),
//     dS^T = P^T o (dP^T - D); the row statistics (max, 1 / sum, D) go to LDS,
//     dQ^T = scale K^T dS^T  (A = K^T from a transposed LDS copy, B = dS^T from the accumulators),
//     dS in float32 to LDS [key][query]; after the pass lane i sums the (q, k) pairs of
//     relative-position index i, 64 + 64 + 41 indices, in a fixed order (this item's dtable).
//   pass 2, per key tile (lane r = key, registers = queries):
//     S = Q K^T, P = exp(s - max_q) / sum_q from the saved statistics, dP = dO V^T, dS,
//     dV^T = dO^T P (P rounded to the operand dtype as the forward rounds it), dK^T = scale Q^T dS
//     (A = dO^T / Q^T from transposed LDS copies that reuse pass 1's LDS).
// A padded-map token has no row: its dK / dV rows are summed per item (fixed shuffle tree over
// the 16 key lanes) into the item's dbk / dbv partial; as a query its dO is zero (its output row
// is cropped), so it contributes nothing and dQ needs no bias partial.  Each real token belongs
// to exactly one window: dq / dk / dv rows are written once, no atomics.  The per-item partials
// [169 + 32 + 32] float32 in the workspace are summed over (image, window) by k_swin_bwd_reduce
// in a fixed order: no float atomics anywhere, bitwise reproducible.
constexpr int SWB_CELLS = SW_TABLE + 2 * SW_HD;  // per-item partials: dtable | dbk | dbv
constexpr int SWB_RSLICES = 16;

struct SwinBwdArgs {
  const void *q, *k, *v;
  long long ldq;
  const float *bq, *bk, *bv;
  const float* table;
  const void* dout;  // [B*H*W][ldo]
  long long ldo;
  void *dq, *dk, *dv;  // rows with stride ldd
  long long ldd;
  float* ws;  // [items][SWB_CELLS]
  int B, H, W, heads, shift, Hp, Wp, nwy, nwx;
  float scale;
};

template <typename T> struct SwB {
  static constexpr int WAVES = sizeof(T) == 2 ? 4 : 2;  // LDS: 4 x 15.8 KB (bf16), 2 x 19.8 KB (f32)
  static constexpr int TILE = SW_HD * SwT<T>::VT_S * (int)sizeof(T);  // one transposed [32][64 + pad] copy
  static constexpr int DSL = (SW_T * SW_T * 4 + 15) / 16 * 16;        // dS float32 [49 keys][49 queries]
  static constexpr int REGION = DSL + TILE > 2 * TILE ? DSL + TILE : 2 * TILE;
};

template <typename T>
__global__ __launch_bounds__(64 * SwB<T>::WAVES) void k_swin_attn_bwd(SwinBwdArgs a) {
  constexpr int WAVES = SwB<T>::WAVES, XS = SwT<T>::VT_S;
  __shared__ __attribute__((aligned(16))) unsigned char region[WAVES][SwB<T>::REGION];
  __shared__ float tab[WAVES][SW_TABLE + 3];
  __shared__ float stat[WAVES][3][64];  // per query: max, 1 / sum, D
  __shared__ int trow[WAVES][64], treg[WAVES][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long item = (long long)blockIdx.x * WAVES + wv;
  const long long total = (long long)a.B * a.nwy * a.nwx * a.heads;
  if (item >= total) return;  // wave-uniform; no workgroup barrier below
  const int h = (int)(item % a.heads);
  long long rest = item / a.heads;
  const int wx = (int)(rest % a.nwx);
  rest /= a.nwx;
  const int wy = (int)(rest % a.nwy);
  const int b = (int)(rest / a.nwy);
  const int r = lane & 15, g = lane >> 4;
  float* tb = tab[wv];
  float(*st)[64] = stat[wv];
  int *tr = trow[wv], *tg = treg[wv];
  for (int i = lane; i < SW_TABLE; i += 64) tb[i] = a.table[i * a.heads + h];
  {  // token t = lane of the window -> original row (-1: padded-map position or t >= 49), shift region
    int row = -1, reg = 0;
    if (lane < SW_T) {
      const int ti = lane / SW_WS, tj = lane % SW_WS;
      const int ys = wy * SW_WS + ti, xs = wx * SW_WS + tj;
      if (a.shift > 0) reg = 3 * sw_region(ys, a.Hp, a.shift) + sw_region(xs, a.Wp, a.shift);
      const int py = a.shift > 0 ? (ys + a.shift) % a.Hp : ys, px = a.shift > 0 ? (xs + a.shift) % a.Wp : xs;
      if (py < a.H && px < a.W) row = (b * a.H + py) * a.W + px;
    }
    tr[lane] = row;
    tg[lane] = reg;
  }
  __builtin_amdgcn_wave_barrier();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

  // 8 consecutive head dims (8g..8g+7) of token t's row of base; a padded token is the bias
  // (pad_bias) or zero, t >= 49 zero.  The load is unconditional on a clamped row, as the forward's.
  auto frag_of = [&](const void* base, long long ld, const float* bias, int t, bool pad_bias) -> Frag<T> {
    Frag<T> f;
    const int row = tr[t];
    const int d0 = h * SW_HD + 8 * g;
    f.load(reinterpret_cast<const T*>(base) + (long long)(row >= 0 ? row : 0) * ld + d0);
    if (row < 0) {
      if (t >= SW_T || !pad_bias) {
        f.zero();
      } else {
        float e[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] = bias ? bias[d0 + j] : 0.f;
        f.from8(e);
      }
    }
    return f;
  };
  // X^T into LDS: lane = token, its 32 dims as four 8-dim fragments (the forward's V^T copy)
  auto fill_t = [&](T* dst, const void* base, long long ld, const float* bias, bool pad_bias) {
    const int t = lane, row = tr[t];
    Frag<T> fx[4];
#pragma unroll
    for (int c = 0; c < 4; ++c)
      fx[c].load(reinterpret_cast<const T*>(base) + (long long)(row >= 0 ? row : 0) * ld + h * SW_HD + 8 * c);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int d0 = h * SW_HD + 8 * c;
      float e[8];
      fx[c].to8(e);
      if (row < 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          e[j] = t < SW_T && pad_bias && bias ? Num<T>::to_f(Num<T>::from_f(bias[d0 + j])) : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) dst[(8 * c + j) * XS + t] = Num<T>::from_f(e[j]);
    }
  };
  // A operand from a transposed copy: dims 16 dt + r, tokens 32 kp + 4g + 0..3 and 32 kp + 16 + 4g +
  // 0..3 — the order of a B operand taken from two accumulator tiles
  auto frag_t = [&](const T* src, int dt, int kp) -> Frag<T> {
    const T* row = src + (16 * dt + r) * XS;
    float e8[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      e8[e] = Num<T>::to_f(row[32 * kp + 4 * g + e]);
      e8[4 + e] = Num<T>::to_f(row[32 * kp + 16 + 4 * g + e]);
    }
    Frag<T> f;
    f.from8(e8);
    return f;
  };
  auto acc_frag = [&](const f32x4& lo, const f32x4& hi) -> Frag<T> {
    float e8[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      e8[e] = lo[e];
      e8[4 + e] = hi[e];
    }
    Frag<T> f;
    f.from8(e8);
    return f;
  };
  auto store4 = [&](void* base, int row, int d0, const f32x4& o, float mul) {
    T* dst = reinterpret_cast<T*>(base) + (long long)row * a.ldd + d0;
    if constexpr (sizeof(T) == 2) {
      *reinterpret_cast<uint2*>(dst) = make_uint2(pack_bf16x2(o[0] * mul, o[1] * mul), pack_bf16x2(o[2] * mul, o[3] * mul));
    } else {
      *reinterpret_cast<float4*>(dst) = make_float4(o[0] * mul, o[1] * mul, o[2] * mul, o[3] * mul);
    }
  };

  // ---- pass 1: query tiles
  {
    float* dsl = reinterpret_cast<float*>(region[wv]);
    T* kt = reinterpret_cast<T*>(region[wv] + SwB<T>::DSL);
    fill_t(kt, a.k, a.ldq, a.bk, true);
    Frag<T> kf[4], vf[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      kf[j] = frag_of(a.k, a.ldq, a.bk, 16 * j + r, true);
      vf[j] = frag_of(a.v, a.ldq, a.bv, 16 * j + r, true);
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    for (int qi = 0; qi < 4; ++qi) {
      const int tq = 16 * qi + r;
      const bool qok = tq < SW_T;
      const int qrow = tr[tq], qreg = tg[tq];
      const Frag<T> qf = frag_of(a.q, a.ldq, a.bq, tq, true);
      const Frag<T> dof = frag_of(a.dout, a.ldo, nullptr, tq, false);
      const int qy = tq / SW_WS, qx = tq % SW_WS;
      f32x4 s[4], dp[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        s[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        dp[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        mma(s[j], kf[j], qf);
        mma(dp[j], vf[j], dof);
      }
      float mx = -INFINITY;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int tk = 16 * j + 4 * g + e;
          float v = -INFINITY;
          if (tk < SW_T) {
            float bm = 0.f;  // a query >= 49 is all zeros: a uniform row, finite statistics, dS = 0
            if (qok) {
              const int ky = tk / SW_WS, kx = tk % SW_WS;
              const int idx = (qy - ky + SW_WS - 1) * (2 * SW_WS - 1) + (qx - kx + SW_WS - 1);
              bm = tb[idx] + (a.shift > 0 && tg[tk] != qreg ? -100.f : 0.f);
            }
            v = s[j][e] * a.scale + bm;
          }
          s[j][e] = v;
          mx = fmaxf(mx, v);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 16));
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      float l = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float p = s[j][e] == -INFINITY ? 0.f : expf(s[j][e] - mx);
          s[j][e] = p;
          l += p;
        }
      l += __shfl_xor(l, 16);
      l += __shfl_xor(l, 32);
      const float inv = 1.f / l;
      float D = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          s[j][e] *= inv;
          dp[j][e] = Num<T>::to_f(Num<T>::from_f(dp[j][e]));
          D += s[j][e] * dp[j][e];
        }
      D += __shfl_xor(D, 16);
      D += __shfl_xor(D, 32);
      if (g == 0) {
        st[0][tq] = mx;
        st[1][tq] = inv;
        st[2][tq] = D;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int tk = 16 * j + 4 * g + e;
          const float ds = s[j][e] * (dp[j][e] - D);
          s[j][e] = ds;
          if (qok && tk < SW_T) dsl[tk * SW_T + tq] = ds;
        }
      Frag<T> dsf[2];
#pragma unroll
      for (int kp = 0; kp < 2; ++kp) dsf[kp] = acc_frag(s[2 * kp], s[2 * kp + 1]);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kp = 0; kp < 2; ++kp) mma(o, frag_t(kt, dt, kp), dsf[kp]);
        // o[e] = dQ^T[dim 16 dt + 4 g + e][query tq] / scale
        if (qrow >= 0) store4(a.dq, qrow, h * SW_HD + 16 * dt + 4 * g, o, a.scale);
      }
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    // this item's dtable: relative-position index i = (qy - ky + 6) * 13 + (qx - kx + 6)
    for (int i = lane; i < SW_TABLE; i += 64) {
      const int dy = i / (2 * SW_WS - 1) - (SW_WS - 1), dx = i % (2 * SW_WS - 1) - (SW_WS - 1);
      float acc = 0.f;
      for (int ky = dy < 0 ? -dy : 0; ky < SW_WS && ky + dy < SW_WS; ++ky)
        for (int kx = dx < 0 ? -dx : 0; kx < SW_WS && kx + dx < SW_WS; ++kx)
          acc += dsl[(ky * SW_WS + kx) * SW_T + (ky + dy) * SW_WS + kx + dx];
      a.ws[item * SWB_CELLS + i] = acc;
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }

  // ---- pass 2: key tiles (Q^T and dO^T reuse pass 1's LDS)
  {
    T* qt = reinterpret_cast<T*>(region[wv]);
    T* dot = reinterpret_cast<T*>(region[wv] + SwB<T>::TILE);
    fill_t(qt, a.q, a.ldq, a.bq, true);
    fill_t(dot, a.dout, a.ldo, nullptr, false);
    Frag<T> qf[4], dof[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      qf[i] = frag_of(a.q, a.ldq, a.bq, 16 * i + r, true);
      dof[i] = frag_of(a.dout, a.ldo, nullptr, 16 * i + r, false);
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    float accbk[2][4], accbv[2][4];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int e = 0; e < 4; ++e) accbk[dt][e] = accbv[dt][e] = 0.f;
    for (int kj = 0; kj < 4; ++kj) {
      const int tk = 16 * kj + r;
      const bool kok = tk < SW_T;
      const int krow = tr[tk], kreg = tg[tk];
      const Frag<T> kf = frag_of(a.k, a.ldq, a.bk, tk, true);
      const Frag<T> vf = frag_of(a.v, a.ldq, a.bv, tk, true);
      const int ky = tk / SW_WS, kx = tk % SW_WS;
      f32x4 s[4], dp[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        s[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        dp[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        mma(s[i], qf[i], kf);
        mma(dp[i], dof[i], vf);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int tq = 16 * i + 4 * g + e;
          float p = 0.f, ds = 0.f;
          if (kok) {
            float bm = 0.f;
            if (tq < SW_T) {
              const int qy = tq / SW_WS, qx = tq % SW_WS;
              const int idx = (qy - ky + SW_WS - 1) * (2 * SW_WS - 1) + (qx - kx + SW_WS - 1);
              bm = tb[idx] + (a.shift > 0 && tg[tq] != kreg ? -100.f : 0.f);
            }
            p = expf(s[i][e] * a.scale + bm - st[0][tq]) * st[1][tq];
            ds = p * (Num<T>::to_f(Num<T>::from_f(dp[i][e])) - st[2][tq]);
          }
          s[i][e] = p;
          dp[i][e] = ds;
        }
      Frag<T> pf[2], dsf[2];
#pragma unroll
      for (int kp = 0; kp < 2; ++kp) {
        pf[kp] = acc_frag(s[2 * kp], s[2 * kp + 1]);
        dsf[kp] = acc_frag(dp[2 * kp], dp[2 * kp + 1]);
      }
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        f32x4 ov = {0.f, 0.f, 0.f, 0.f}, ok = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kp = 0; kp < 2; ++kp) {
          mma(ov, frag_t(dot, dt, kp), pf[kp]);
          mma(ok, frag_t(qt, dt, kp), dsf[kp]);
        }
        // ov[e] = dV^T[dim 16 dt + 4 g + e][key tk], ok[e] = dK^T[..][key tk] / scale
        if (krow >= 0) {
          store4(a.dv, krow, h * SW_HD + 16 * dt + 4 * g, ov, 1.f);
          store4(a.dk, krow, h * SW_HD + 16 * dt + 4 * g, ok, a.scale);
        } else if (kok) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            accbv[dt][e] += ov[e];
            accbk[dt][e] += ok[e] * a.scale;
          }
        }
      }
    }
    // the padded keys' rows summed over the 16 key lanes (fixed tree), one partial per item
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float vk = accbk[dt][e], vv = accbv[dt][e];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          vk += __shfl_xor(vk, o);
          vv += __shfl_xor(vv, o);
        }
        if (r == 0) {
          a.ws[item * SWB_CELLS + SW_TABLE + 16 * dt + 4 * g + e] = vk;
          a.ws[item * SWB_CELLS + SW_TABLE + SW_HD + 16 * dt + 4 * g + e] = vv;
        }
      }
  }
}

// dtable[c][h] / dbk[32 h + c'] / dbv[32 h + c'] = sum over the (image, window) items of head h of
// partial cell c: SWB_RSLICES strided slices per cell, each summed in item order, then the slices
// in order.  grid (ceil(233 / 64), heads), block (64, SWB_RSLICES).
__global__ __launch_bounds__(64 * SWB_RSLICES) void k_swin_bwd_reduce(const float* ws, long long nbw, int heads,
                                                                      float* dtable, float* dbk, float* dbv) {
  __shared__ float red[SWB_RSLICES][64];
  const int c = blockIdx.x * 64 + threadIdx.x, h = blockIdx.y;
  float acc = 0.f;
  if (c < SWB_CELLS)
    for (long long i = threadIdx.y; i < nbw; i += SWB_RSLICES) acc += ws[(i * heads + h) * SWB_CELLS + c];
  red[threadIdx.y][threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.y != 0 || c >= SWB_CELLS) return;
  float sum = red[0][threadIdx.x];
  for (int s = 1; s < SWB_RSLICES; ++s) sum += red[s][threadIdx.x];
  if (c < SW_TABLE) {
    dtable[c * heads + h] = sum;
  } else if (c < SW_TABLE + SW_HD) {
    if (dbk) dbk[h * SW_HD + c - SW_TABLE] = sum;
  } else {
    if (dbv) dbv[h * SW_HD + c - SW_TABLE - SW_HD] = sum;
  }
}

}  // namespace
}  // namespace rgbd

using namespace rgbd;

extern "C" {

size_t rgbd_swin_window_attn_bwd_workspace_size(int B, int H, int W, int heads) {
  if (B <= 0 || H <= 0 || W <= 0 || heads <= 0) return 0;
  const size_t nw = (size_t)((H + SW_WS - 1) / SW_WS) * (size_t)((W + SW_WS - 1) / SW_WS);
  return align256((size_t)B * nw * (size_t)heads * SWB_CELLS * sizeof(float));
}

int rgbd_swin_window_attn_bwd(int dtype, const void* q, const void* k, const void* v, long long ldq, const float* bq,
                              const float* bk, const float* bv, const float* table, const void* dout, long long ldo,
                              int B, int H, int W, int heads, int window, int shift, float scale, void* dq, void* dk,
                              void* dv, long long ldd, float* dbk, float* dbv, float* dtable, void* ws,
                              void* stream) {
  RGBD_REQUIRE(q && k && v && table && dout && dq && dk && dv && dtable && ws, RGBD_E_ARG);
  RGBD_REQUIRE(B > 0 && H > 0 && W > 0 && heads > 0, RGBD_E_ARG);
  RGBD_REQUIRE(window == SW_WS && shift >= 0 && shift < SW_WS, RGBD_E_SHAPE);
  RGBD_REQUIRE((long long)B * H * W <= 0x7fffffffLL, RGBD_E_SHAPE);
  const long long C = (long long)heads * SW_HD;
  RGBD_REQUIRE(ldq >= C && ldo >= C && ldd >= C, RGBD_E_SHAPE);
  RGBD_REQUIRE(dtype == RGBD_BF16 || dtype == RGBD_F32, RGBD_E_DTYPE);
  const int esz = dtype == RGBD_BF16 ? 2 : 4;
  RGBD_REQUIRE((ldq * esz) % 16 == 0 && (ldo * esz) % 16 == 0 && (ldd * esz) % 16 == 0, RGBD_E_SHAPE);
  RGBD_REQUIRE(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)dout | (uintptr_t)dq | (uintptr_t)dk |
                (uintptr_t)dv) % 16 == 0 && (uintptr_t)ws % 4 == 0, RGBD_E_SHAPE);
  SwinBwdArgs a;
  a.q = q; a.k = k; a.v = v; a.ldq = ldq;
  a.bq = bq; a.bk = bk; a.bv = bv; a.table = table;
  a.dout = dout; a.ldo = ldo;
  a.dq = dq; a.dk = dk; a.dv = dv; a.ldd = ldd;
  a.ws = reinterpret_cast<float*>(ws);
  a.B = B; a.H = H; a.W = W; a.heads = heads; a.shift = shift;
  a.Hp = (H + SW_WS - 1) / SW_WS * SW_WS;
  a.Wp = (W + SW_WS - 1) / SW_WS * SW_WS;
  a.nwy = a.Hp / SW_WS; a.nwx = a.Wp / SW_WS;
  a.scale = scale;
  const long long nbw = (long long)B * a.nwy * a.nwx, items = nbw * heads;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == RGBD_BF16) {
    constexpr int WV = SwB<bf16_t>::WAVES;
    hipLaunchKernelGGL(k_swin_attn_bwd<bf16_t>, dim3((unsigned)((items + WV - 1) / WV)), dim3(64 * WV), 0, s, a);
  } else {
    constexpr int WV = SwB<float>::WAVES;
    hipLaunchKernelGGL(k_swin_attn_bwd<float>, dim3((unsigned)((items + WV - 1) / WV)), dim3(64 * WV), 0, s, a);
  }
  RGBD_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_swin_bwd_reduce, dim3((SWB_CELLS + 63) / 64, heads), dim3(64, SWB_RSLICES), 0, s, a.ws, nbw,
                     heads, dtable, dbk, dbv);
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

int rgbd_swin_window_attn(int dtype, const void* q, const void* k, const void* v, long long ldq, const float* bq,
                          const float* bk, const float* bv, const float* table, int B, int H, int W, int heads,
                          int window, int shift, float scale, void* out, long long ldo, void* stream) {
  RGBD_REQUIRE(q && k && v && table && out && B > 0 && H > 0 && W > 0 && heads > 0, RGBD_E_ARG);
  RGBD_REQUIRE(window == SW_WS && shift >= 0 && shift < SW_WS, RGBD_E_SHAPE);
  RGBD_REQUIRE(ldq >= (long long)heads * SW_HD && ldo >= (long long)heads * SW_HD, RGBD_E_SHAPE);
  const int esz = dtype == RGBD_BF16 ? 2 : 4;
  RGBD_REQUIRE((ldq * esz) % 16 == 0 && (ldo * esz) % 16 == 0, RGBD_E_SHAPE);
  RGBD_REQUIRE(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) % 16 == 0, RGBD_E_SHAPE);
  SwinArgs a;
  a.q = q; a.k = k; a.v = v; a.ldq = ldq;
  a.bq = bq; a.bk = bk; a.bv = bv; a.table = table;
  a.out = out; a.ldo = ldo;
  a.B = B; a.H = H; a.W = W; a.heads = heads; a.shift = shift;
  a.Hp = (H + SW_WS - 1) / SW_WS * SW_WS;
  a.Wp = (W + SW_WS - 1) / SW_WS * SW_WS;
  a.nwy = a.Hp / SW_WS; a.nwx = a.Wp / SW_WS;
  a.scale = scale;
  const long long items = (long long)B * a.nwy * a.nwx * heads;
  const int blocks = (int)((items + SW_WAVES - 1) / SW_WAVES);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == RGBD_BF16)
    hipLaunchKernelGGL(k_swin_attn<bf16_t>, dim3(blocks), dim3(64 * SW_WAVES), 0, s, a);
  else if (dtype == RGBD_F32)
    hipLaunchKernelGGL(k_swin_attn<float>, dim3(blocks), dim3(64 * SW_WAVES), 0, s, a);
  else
    return RGBD_E_DTYPE;
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

}  // extern "C"
