// K4: EnhancedDepthImageRatioPredictor (mask2former/utils/custom_model.py:1363-1487) on gfx950.
//
// 216 GFLOP/img at 640x480 — the FLOP-dominant row of the hot path (SURVEY Finding 1).
// One float32 depth image [3,H,W] in, one ratio out:
//   chain  : per pixel, three chained MFMA GEMMs.  stem = the three 'same' convs 3x3 / 5x5 / 7x7
//            (3->64 each, :1378-1394) merged into ONE 7x7 conv 3->192 (3x3 and 5x5 kernels embedded
//            at the centre, zero elsewhere; torch.cat order of :1463 preserved); fusion = 1x1
//            192->128 (:1397-1401); attention 1x1 128->64 ->ReLU-> 64->128 ->sigmoid and the gate
//            (:1404-1470).  Each GEMM's accumulator (channel in the registers, pixel on the lane)
//            is directly the next GEMM's B operand; the packed weights use the matching k
//            permutation (chain_perm).
//   conv5  : 3x3 128->256 (:1413), 84 % of the FLOPs, LDS-tiled implicit GEMM
//   pool   : BN + ReLU + AdaptiveAvgPool(4)
//   tail   : 3x3 256->512 on 4x4 + BN + ReLU + GAP, MLP + dropout + sigmoid,
//            ratio = 0.01 + 0.49 sigmoid(raw) (:1485).
// BatchNorm (six layers: stem x 3, fusion, conv5, tail conv): eval mode uses the running
// statistics; train mode the batch statistics (deterministic fixed-order reductions, double across
// workgroups) and updates the running statistics like torch (momentum, unbiased variance).
// Dropout uses a counter-hash RNG (train mode only).
//
// Files: this one holds the weight packing (k_rp_pack), the workspace carve, the two forwards
// below and the C ABI; the kernels are in the stage files, each behind a few host launch functions
// declared in ratio_common.hpp:
//   ratio_stem.hip   k_bn_affine, k_bn_affine_stem, k_stem_lag, k_stem_sums, k_stem_s2, k_stem_bn
//   ratio_chain.hip  k_rp_fold, k_rp_chain_v2<phase>
//   ratio_conv5.hip  k_rp_gate, k_c4_pad_zero, k_rp_conv5_v4<mode>, k_rp_bn_relu_pool_v4_tiles,
//                    k_rp_bn_relu_pool_v4_frag, k_rp_pool_finish_v4
//   ratio_f32.hip    k_rp_chain<phase>, k_rp_conv3x3, k_rp_bn_relu_pool
//   ratio_tail.hip   k_rp_pool_finish, k_rp_tail_convbn, k_rp_tail_fc1, k_rp_tail_head
//
// Launch sequences ([train] = train mode only):
//   float32 (forward_f32), train and eval:
//     [train] k_rp_chain<0> -> k_bn_affine_stem -> [train] k_rp_chain<1> -> k_bn_affine (fusion) ->
//     k_rp_chain<2> -> k_rp_conv3x3 -> k_bn_affine (conv5) -> k_rp_bn_relu_pool -> k_rp_pool_finish
//     -> tail
//   bf16 train (forward_bf16):
//     k_stem_lag -> k_stem_sums -> k_stem_s2 -> k_stem_bn (stem BN affines from the moments of the
//     depth windows, + the BN1 fold and conv5's input padding) -> k_rp_chain_v2<1> (fusion
//     statistics + the raw fusion output) -> k_bn_affine (fusion) -> k_rp_gate -> k_rp_conv5_v4<0>
//     -> k_bn_affine (conv5) -> k_rp_bn_relu_pool_v4_tiles | _frag -> k_rp_pool_finish -> tail
//     (images under 8 pixels a side: k_rp_chain_v2<0> -> k_bn_affine_stem -> k_rp_fold(1) ->
//     k_c4_pad_zero instead of the four stem kernels; RGBD_RATIO_F_PHASE2: k_rp_fold(2) ->
//     k_rp_chain_v2<2> instead of k_rp_gate)
//   bf16 eval (forward_bf16):
//     k_bn_affine_stem -> k_rp_fold(1) -> k_c4_pad_zero -> k_bn_affine (fusion) -> k_rp_fold(2) ->
//     k_rp_chain_v2<2> -> k_bn_affine (conv5) -> k_rp_conv5_v4<1> -> k_rp_pool_finish_v4 -> tail,
//     or, where the pool does not fuse into conv5's epilogue (conv4_pool_fused): k_rp_conv5_v4<2>
//     -> k_rp_bn_relu_pool_v4_tiles | _frag -> k_rp_pool_finish -> tail
//   tail (both): k_rp_tail_convbn -> k_rp_tail_fc1 -> k_rp_tail_head
#include "ratio_common.hpp"

using namespace rgbd;
using namespace rgbd::rp;

namespace {

// ------------------------------------------------------------------ packing
template <typename T>
__global__ void k_rp_pack(WPtrs w, char* blob, Layout L) {
  const int tid = blockIdx.x * blockDim.x + threadIdx.x, nth = gridDim.x * blockDim.x;
  T* w1 = (T*)(blob + L.w1);
  float* b1 = (float*)(blob + L.b1);
  for (int e = tid; e < STEM_C * STEM_K; e += nth) {  // stem: k = tap*3 + c over a 7x7 window
    const int o = e / STEM_K, k = e % STEM_K;
    float v = 0.f;
    if (k < 147) {
      const int tap = k / 3, c = k % 3, ky = tap / 7, kx = tap % 7;
      const int br = o / 64, oo = o % 64, ks = 3 + 2 * br, off = 3 - ks / 2;  // 3x3 / 5x5 / 7x7
      const int y = ky - off, x = kx - off;
      if (y >= 0 && y < ks && x >= 0 && x < ks) v = w.p[2 * br][((oo * 3 + c) * ks + y) * ks + x];
    }
    w1[e] = Num<T>::from_f(v);
  }
  for (int e = tid; e < STEM_C; e += nth) b1[e] = w.p[2 * (e / 64) + 1][e % 64];
  // chained 1x1 layers: packed[o][32s + 8g + e] = W[o][32s + perm(g, e)]
  auto pack_chain = [&](const float* src, T* dst, int O, int K) {
    for (int e = tid; e < O * K; e += nth) {
      const int o = e / K, kk = e % K, s = kk / 32, g = (kk % 32) / 8, ee = kk % 8;
      dst[e] = Num<T>::from_f(src[o * K + 32 * s + chain_perm(g, ee)]);
    }
  };
  pack_chain(w.p[6], (T*)(blob + L.w2), FUS_C, STEM_C);
  pack_chain(w.p[8], (T*)(blob + L.w3), ATT_C, FUS_C);
  pack_chain(w.p[10], (T*)(blob + L.w4), FUS_C, ATT_C);
  for (int e = tid; e < FUS_C; e += nth) ((float*)(blob + L.b2))[e] = w.p[7][e];
  for (int e = tid; e < ATT_C; e += nth) ((float*)(blob + L.b3))[e] = w.p[9][e];
  for (int e = tid; e < FUS_C; e += nth) ((float*)(blob + L.b4))[e] = w.p[11][e];
  // conv5 [256][9][128] (k = tap*128 + c) from [256][128][3][3]
  T* w5 = (T*)(blob + L.w5);
  for (int e = tid; e < C5 * 9 * FUS_C; e += nth) {
    const int o = e / (9 * FUS_C), tap = (e / FUS_C) % 9, c = e % FUS_C;
    w5[e] = Num<T>::from_f(w.p[12][(o * FUS_C + c) * 9 + tap]);
  }
  for (int e = tid; e < C5; e += nth) ((float*)(blob + L.b5))[e] = w.p[13][e];
  if constexpr (sizeof(T) == 2) {
    bf16_t* w1s = (bf16_t*)(blob + L.w1s);
    for (int e = tid; e < STEM_C * STEM_K2; e += nth) {  // stem for chain v2: k = (c*7 + ky)*8 + kx
      const int o = e / STEM_K2, k = e % STEM_K2, grp = k / 8, kx = k % 8, c = grp / 7, ky = grp % 7;
      float v = 0.f;
      if (kx < 7) {
        const int br = o / 64, oo = o % 64, ks = 3 + 2 * br, off = 3 - ks / 2;  // 3x3 / 5x5 / 7x7
        const int y = ky - off, x = kx - off;
        if (y >= 0 && y < ks && x >= 0 && x < ks) v = w.p[2 * br][((oo * 3 + c) * ks + y) * ks + x];
      }
      w1s[e] = f32_to_bf16(v);
      ((float*)(blob + L.w1f))[e] = v;
    }
    for (int e = tid; e < FUS_C * STEM_C; e += nth) {  // f32 fusion weights in the chain order
      const int o = e / STEM_C, kk = e % STEM_C, s = kk / 32, g = (kk % 32) / 8, ee = kk % 8;
      ((float*)(blob + L.w2f))[e] = w.p[6][o * STEM_C + 32 * s + chain_perm(g, ee)];
    }
    // k_rp_conv5_v4: [half][step = quarter*3 + ky][kx][n][32 ch] (64-byte rows, chunk slot s <-
    // chunk s ^ ((n >> 1) & 2)): one step of one channel half is one linear 24 KiB copy
    bf16_t* w5q = (bf16_t*)(blob + L.w5q);
    for (int e = tid; e < C5 * 9 * FUS_C; e += nth) {
      const int k8 = e % 8, sl = (e / 8) % 4, n = (e / 32) % 128, kx = (e / 4096) % 3, st = (e / 12288) % 12,
                nh = e / 147456;
      const int qt = st / 3, ky = st % 3, c = 32 * qt + 8 * (sl ^ ((n >> 1) & 2)) + k8;
      w5q[e] = f32_to_bf16(w.p[12][((nh * 128 + n) * FUS_C + c) * 9 + ky * 3 + kx]);
    }
  }
  for (int e = tid; e < 64; e += nth) ((float*)(blob + L.zero))[e] = 0.f;
  // tail + MLP stay float32 in reference layout
  auto copy = [&](const float* src, size_t off, int n) {
    for (int e = tid; e < n; e += nth) ((float*)(blob + off))[e] = src[e];
  };
  copy(w.p[14], L.w6, C6 * C5 * 9);
  copy(w.p[15], L.b6, C6);
  copy(w.p[16], L.w7, 128 * 512);
  copy(w.p[17], L.b7, 128);
  copy(w.p[18], L.w8, 64 * 128);
  copy(w.p[19], L.b8, 64);
  copy(w.p[20], L.w9, 32 * 64);
  copy(w.p[21], L.b9, 32);
  copy(w.p[22], L.w10, 32);
  copy(w.p[23], L.b10, 1);
}

struct Ws {  // workspace carve
  size_t aff1, aff2, aff5, slab, att, y, part, pooled, feat, h1, fold, stem, total;
};

inline Ws make_ws(int es, int B, int H, int W) {
  Ws w;
  size_t o = 0;
  auto seg = [&](size_t bytes) {
    size_t r = o;
    o += align256(bytes);
    return r;
  };
  const size_t P = (size_t)B * H * W;
  const int slab_rows = std::max(std::max(chain_grid(B, H, W), 8 * chain_grid_v2(B, H, W, 0)),
                                 std::max(conv_grid(B, H, W), conv4_grid(B, H, W)));
  w.aff1 = seg(STEM_C * sizeof(float2));
  w.aff2 = seg(FUS_C * sizeof(float2));
  w.aff5 = seg(C5 * sizeof(float2));
  w.slab = seg((size_t)slab_rows * C5 * 2 * sizeof(float));
  w.att = seg(es == 2 ? (size_t)B * c4_ph(H) * c4_pw(W) * FUS_C * 2 : P * FUS_C * es);
  w.y = seg(es == 2 ? (size_t)conv4_tiles(B, H, W) * C4_TH * C4_TW * C5 * 2 : P * C5 * es);
  w.part = seg((size_t)B * 16 * POOL_SPLIT * C5 * sizeof(float));
  w.pooled = seg((size_t)B * C5 * 16 * sizeof(float));
  w.feat = seg((size_t)B * C6 * sizeof(float));
  w.h1 = seg((size_t)B * 128 * sizeof(float));
  w.fold = seg(es == 2 ? FOLD_BYTES : 0);
  w.stem = seg(es == 2 && stem_moments_ok(H, W) ? stem_ws_size(B, H, W) : 0);
  w.total = o;
  return w;
}

// the carve for the C-ABI size / offset entry points (a non-positive extent counts as 1)
Ws abi_ws(int dtype, int B, int H, int W) {
  return make_ws(dtype == RGBD_BF16 ? 2 : 4, B > 0 ? B : 1, H > 0 ? H : 1, W > 0 ? W : 1);
}

struct Fwd {  // rgbd_ratio_forward's arguments, checked
  int training;
  float momentum;
  const float* depth3;
  long long bstride;
  int B, H, W;
  const char* blob;
  BnPtrs bn;
  unsigned long long seed, *seed_ctr;
  float* ratio;
  char* ws;
  int flags;
  hipStream_t s;
};

#define RP_TRY(call)                   \
  do {                                 \
    const int e__ = (call);            \
    if (e__ != RGBD_OK) return e__;    \
  } while (0)

// float32 parity path (ratio_f32.hip kernels): every BN from a statistics pass of its own
int forward_f32(const Fwd& a) {
  const int training = a.training, B = a.B, H = a.H, W = a.W;
  const Layout L = make_layout(4);
  const Ws w = make_ws(4, B, H, W);
  float2 *aff1 = (float2*)(a.ws + w.aff1), *aff2 = (float2*)(a.ws + w.aff2), *aff5 = (float2*)(a.ws + w.aff5);
  float *slab = (float*)(a.ws + w.slab), *att = (float*)(a.ws + w.att), *y = (float*)(a.ws + w.y);
  float *part = (float*)(a.ws + w.part), *pooled = (float*)(a.ws + w.pooled);
  const double P = (double)B * H * W;
  const int gch = chain_grid(B, H, W);
  if (training) RP_TRY(chain_f32(0, a.depth3, a.bstride, B, H, W, a.blob, L, nullptr, nullptr, slab, nullptr, a.s));
  RP_TRY(bn_affine_stem(slab, gch, P, training, a.momentum, a.bn, aff1, a.s));
  if (training) RP_TRY(chain_f32(1, a.depth3, a.bstride, B, H, W, a.blob, L, aff1, nullptr, slab, nullptr, a.s));
  RP_TRY(bn_affine(slab, gch, FUS_C, P, training, a.momentum, a.bn, 3, aff2, 0, a.s));
  RP_TRY(chain_f32(2, a.depth3, a.bstride, B, H, W, a.blob, L, aff1, aff2, nullptr, att, a.s));
  RP_TRY(conv3x3_f32(att, B, H, W, a.blob, L, y, slab, a.s));
  RP_TRY(bn_affine(slab, conv_grid(B, H, W), C5, P, training, a.momentum, a.bn, 4, aff5, 0, a.s));
  RP_TRY(bn_relu_pool_f32(y, B, H, W, aff5, part, a.s));
  RP_TRY(pool_finish(part, B, H, W, pooled, a.s));
  return tail(pooled, B, training, a.momentum, a.blob, L, a.bn, a.seed, a.seed_ctr, (float*)(a.ws + w.feat),
              (float*)(a.ws + w.h1), a.ratio, a.s);
}

// bf16 hot path.  Train: stem moments -> chain phase 1 -> gate -> conv5 MODE 0 -> pool; eval: the
// running-statistics affines folded into the weights -> chain phase 2 -> conv5 MODE 1 | 2.
int forward_bf16(const Fwd& a) {
  const int training = a.training, B = a.B, H = a.H, W = a.W;
  const Layout L = make_layout(2);
  const Ws w = make_ws(2, B, H, W);
  float2 *aff1 = (float2*)(a.ws + w.aff1), *aff2 = (float2*)(a.ws + w.aff2), *aff5 = (float2*)(a.ws + w.aff5);
  float *slab = (float*)(a.ws + w.slab), *part = (float*)(a.ws + w.part), *pooled = (float*)(a.ws + w.pooled);
  bf16_t *att = (bf16_t*)(a.ws + w.att), *y = (bf16_t*)(a.ws + w.y);
  char* fold = a.ws + w.fold;
  const double P = (double)B * H * W;
  // stem BNs (+ the BN1 fold and conv5 v4's input padding)
  if (training && stem_moments_ok(H, W)) {  // the moments of the windows: no stem pass
    RP_TRY(stem_bn_moments(a.depth3, a.bstride, B, H, W, a.blob, L, a.momentum, a.bn, aff1, fold, att, a.ws + w.stem, a.s));
  } else {
    if (training) RP_TRY(chain_v2(0, a.depth3, a.bstride, B, H, W, a.blob, L, nullptr, nullptr, fold, slab, nullptr, a.s));
    RP_TRY(bn_affine_stem(slab, 8 * chain_grid_v2(B, H, W, 0), P, training, a.momentum, a.bn, aff1, a.s));
    RP_TRY(fold_bn(a.blob, L, aff1, 1, fold, a.s));
    RP_TRY(c4_pad_zero(att, B, H, W, a.s));
  }
  // fusion BN.  Train: phase 1 also stores its raw fusion output for k_rp_gate, in conv5's output
  // buffer, which is dead until conv5.  RGBD_RATIO_F_PHASE2: train through phase 2 instead of the
  // gate (a test compares the two routes' gated features).
  const bool use_gate = training && !(a.flags & RGBD_RATIO_F_PHASE2);
  if (training)
    RP_TRY(chain_v2(1, a.depth3, a.bstride, B, H, W, a.blob, L, aff1, nullptr, fold, slab, use_gate ? y : nullptr, a.s));
  RP_TRY(bn_affine(slab, 8 * chain_grid_v2(B, H, W), FUS_C, P, training, a.momentum, a.bn, 3, aff2, 1, a.s));
  if (use_gate) {
    RP_TRY(gate(y, B, H, W, a.blob, L, aff2, att, a.s));
  } else {
    RP_TRY(fold_bn(a.blob, L, aff2, 2, fold, a.s));
    RP_TRY(chain_v2(2, a.depth3, a.bstride, B, H, W, a.blob, L, aff1, aff2, fold, nullptr, att, a.s));
  }
  // conv5 + its BN statistics (train), or BN (running statistics) + ReLU + pool in its epilogue
  // (eval, MODE 1: the per-item bin partials go where y would)
  const int mode = training ? 0 : (conv4_pool_fused(H, W) ? 1 : 2);
  if (!training) RP_TRY(bn_affine(slab, 0, C5, P, 0, a.momentum, a.bn, 4, aff5, 0, a.s));
  RP_TRY(conv5_v4(mode, att, B, H, W, a.blob, L, aff5, y, mode == 0 ? slab : mode == 1 ? (float*)y : nullptr, a.s));
  if (training) RP_TRY(bn_affine(slab, conv4_grid(B, H, W), C5, P, 1, a.momentum, a.bn, 4, aff5, 1, a.s));
  if (mode == 1) {
    RP_TRY(pool_finish_v4((const float*)y, B, H, W, pooled, a.s));
  } else {
    RP_TRY(pool_v4(y, B, H, W, aff5, part, a.s));
    RP_TRY(pool_finish(part, B, H, W, pooled, a.s));
  }
  return tail(pooled, B, training, a.momentum, a.blob, L, a.bn, a.seed, a.seed_ctr, (float*)(a.ws + w.feat),
              (float*)(a.ws + w.h1), a.ratio, a.s);
}

}  // namespace

extern "C" {

size_t rgbd_ratio_packed_size(int dtype) { return make_layout(dtype == RGBD_BF16 ? 2 : 4).total; }

int rgbd_ratio_pack(int dtype, const float* const* weights_host, void* packed, void* stream) {
  RGBD_REQUIRE(weights_host && packed, RGBD_E_ARG);
  WPtrs w;
  for (int i = 0; i < RGBD_RATIO_NW; ++i) {
    RGBD_REQUIRE(weights_host[i], RGBD_E_ARG);
    w.p[i] = weights_host[i];
  }
  hipStream_t s = (hipStream_t)stream;
  if (dtype == RGBD_F32)
    k_rp_pack<float><<<1024, 256, 0, s>>>(w, (char*)packed, make_layout(4));
  else if (dtype == RGBD_BF16)
    k_rp_pack<bf16_t><<<1024, 256, 0, s>>>(w, (char*)packed, make_layout(2));
  else
    return RGBD_E_DTYPE;
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

size_t rgbd_ratio_features_offset(int dtype, int B, int H, int W) {
  return abi_ws(dtype, B, H, W).att;
}

size_t rgbd_ratio_pooled_offset(int dtype, int B, int H, int W) {
  return abi_ws(dtype, B, H, W).pooled;
}

size_t rgbd_ratio_feat_offset(int dtype, int B, int H, int W) {
  return abi_ws(dtype, B, H, W).feat;
}

size_t rgbd_ratio_hidden_offset(int dtype, int B, int H, int W) {
  return abi_ws(dtype, B, H, W).h1;
}

size_t rgbd_ratio_workspace_size(int dtype, int B, int H, int W) {
  return abi_ws(dtype, B, H, W).total;
}

int rgbd_ratio_forward(int dtype, int training, float momentum, const float* depth3, long long batch_stride,
                       int B, int H, int W, const void* packed, float* const* bn_host, unsigned long long seed,
                       unsigned long long* seed_counter, float* ratio, void* ws, int flags, void* stream) {
  RGBD_REQUIRE((flags & ~RGBD_RATIO_F_PHASE2) == 0, RGBD_E_ARG);
  RGBD_REQUIRE(depth3 && packed && bn_host && ratio && ws, RGBD_E_ARG);
  RGBD_REQUIRE(B > 0 && H > 0 && W > 0, RGBD_E_ARG);
  RGBD_REQUIRE(B <= 32, RGBD_E_SHAPE);  // k_rp_tail_fc1 / k_rp_tail_head hold the batch in LDS
  RGBD_REQUIRE((long long)B * ((H + 7) / 8) * ((W + 31) / 32) < (1ll << 30), RGBD_E_SHAPE);  // 32-bit tile indices
  Fwd a{training, momentum, depth3, batch_stride, B, H, W, (const char*)packed, {}, seed, seed_counter,
        ratio, (char*)ws, flags, (hipStream_t)stream};
  for (int i = 0; i < RGBD_RATIO_NBN * 4; ++i) {
    RGBD_REQUIRE(bn_host[i], RGBD_E_ARG);
    a.bn.p[i] = bn_host[i];
  }
  if (dtype == RGBD_F32) return forward_f32(a);
  if (dtype == RGBD_BF16) return forward_bf16(a);
  return RGBD_E_DTYPE;
}

}  // extern "C"
