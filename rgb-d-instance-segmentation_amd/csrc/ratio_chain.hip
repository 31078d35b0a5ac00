// K4 stage file: the bf16 chain (stem 7x7 -> fusion 1x1 -> attention 1x1s -> gate), k_rp_chain_v2,
// and the BN folding that feeds it, k_rp_fold.  Overview: ratio.hip.
#include "ratio_common.hpp"

using namespace rgbd;
using namespace rgbd::rp;

namespace {

// ------------------------------------------------------------------ BN folding (bf16 chain)
// Once the statistics of a BN layer are known, fold its affine (sc, sh) into the producing
// layer: W' = bf16(sc * W_f32) row-wise, b' = sc * b + sh, so the chain applies only the ReLU.
// (fold layout: FOLD_W1 .. FOLD_BYTES above)  which = 1 | 2.
__global__ __launch_bounds__(256) void k_rp_fold(const char* __restrict__ blob, Layout L,
                                                 const float2* __restrict__ aff, int which, char* __restrict__ fold) {
  const int c = blockIdx.x;
  const int K = which == 1 ? STEM_K2 : STEM_C;
  const float* w = (const float*)(blob + (which == 1 ? L.w1f : L.w2f)) + (size_t)c * K;
  bf16_t* wo = (bf16_t*)(fold + (which == 1 ? FOLD_W1 : FOLD_W2)) + (size_t)c * K;
  const float2 a = aff[c];
  for (int k = threadIdx.x; k < K; k += 256) wo[k] = f32_to_bf16(w[k] * a.x);
  if (threadIdx.x == 0) {
    const float b = ((const float*)(blob + (which == 1 ? L.b1 : L.b2)))[c];
    ((float*)(fold + (which == 1 ? FOLD_B1 : FOLD_B2)))[c] = __builtin_fmaf(b, a.x, a.y);
  }
}

// ------------------------------------------------------------------ chain v2 (bf16)
// 512 threads = 8 waves; persistent; ALL chain weights (143 KB bf16) live in LDS for the
// workgroup's lifetime; a wave owns 32 pixels (one row of a 8x32 tile, two 16-px MFMA
// columns) so every weight fragment read from LDS feeds two MFMAs.  BN statistics (phases
// 0/1) are reduced across the wave's 32 pixels and kept per lane in registers, then written
// as one slab row per wave: deterministic.
constexpr int C2W_PWP = 40;  // bf16 patch row: 38 pixels + 2 zero pad (a lane reads 5 words from col & ~1)
constexpr size_t C2W_OFF_W1 = 0;
constexpr size_t C2W_OFF_W2 = C2W_OFF_W1 + (size_t)STEM_C * C2W_S1 * 2;
constexpr size_t C2W_OFF_W3 = C2W_OFF_W2 + (size_t)FUS_C * C2W_S2 * 2;
constexpr size_t C2W_OFF_W4 = C2W_OFF_W3 + (size_t)ATT_C * C2W_S3 * 2;
// Phase 0 (stem statistics) keeps only W1 resident: ~76 KB, two workgroups per CU.
template <int PH> constexpr size_t c2w_off_b() {  // b1 b2 b3 b4 (f32)
  return PH == 0 ? C2W_OFF_W2 : C2W_OFF_W4 + (size_t)FUS_C * C2W_S4 * 2;
}
template <int PH> constexpr size_t c2w_off_aff() {  // aff1, aff2
  return c2w_off_b<PH>() + (size_t)(STEM_C + FUS_C + ATT_C + FUS_C) * 4;
}
template <int PH> constexpr size_t c2w_off_patch() {  // bf16 [3][14][40]
  return c2w_off_aff<PH>() + (size_t)(STEM_C + FUS_C) * 8;
}
template <int PH> constexpr size_t c2w_smem() { return c2w_off_patch<PH>() + (size_t)3 * C2W_PH * C2W_PWP * 2 + 16; }
static_assert(c2w_smem<1>() <= 163840, "chain v2 LDS budget");
// Phase 1 (train: stem + fusion + fusion statistics) needs neither W3 nor W4: their space holds
// eight copies of the depth patch shifted by 0..7 columns, [shift k][3][14][40] with element j of
// copy k = patch column j + k, so the 8 patch values a lane feeds the stem (columns col .. col+7)
// are ONE 16-byte-aligned ds_read_b128 from copy col % 8 (the other phases: 5 dword reads and 4
// byte-aligns per fragment)
constexpr size_t C2W_OFF_P8 = C2W_OFF_W3;
constexpr int C2W_P8 = 8 * 3 * C2W_PH * C2W_PWP;  // bf16 elements
static_assert(C2W_OFF_P8 + (size_t)C2W_P8 * 2 <= c2w_off_b<1>(), "phase-1 shifted patches fit W3 + W4");
static_assert(2 * c2w_smem<0>() <= 163840, "chain v2 phase 0: two workgroups per CU");

// Diagnostics (rgbd_debug_chain_stamps): the STAMPS instantiation records, for workgroup 0's tiles
// 8-11, s_memtime per wave at: tile top, patch staged (after the second barrier), next
// patch's loads issued, stem MFMAs issued (phase 0: statistics done), stem ReLU/pack done, fusion
// MFMAs issued, tile end (statistics + stores): stamps[((phase * 4 + tile) * 8 + wave) * 7 + point].
__device__ unsigned long long* g_c2_stamps = nullptr;
// the stamped instantiations exist only in the diagnostic build (make diag, RGBD_DIAG)
[[maybe_unused]] static bool c2_stamps_on = false;
__device__ __forceinline__ void c2_stamp(unsigned long long* st, long long idx) {
  __builtin_amdgcn_sched_barrier(0);
  const unsigned long long t = __builtin_amdgcn_s_memtime();
  if ((threadIdx.x & 63) == 0) st[idx] = t;
  __builtin_amdgcn_sched_barrier(0);
}

template <int PHASE, bool STAMPS = false>
__global__ __launch_bounds__(512, PHASE == 0 ? 4 : 2) void k_rp_chain_v2(const float* __restrict__ depth3, long long bstride, int B,
                                                     int H, int W, const char* __restrict__ blob, Layout L,
                                                     const float2* __restrict__ aff1, const float2* __restrict__ aff2,
                                                     const char* __restrict__ fold, float* __restrict__ slab,
                                                     bf16_t* __restrict__ att) {
  // phases 1/2 take W1 (and in phase 2 W2) with their BN folded in (k_rp_fold): ReLU only
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const bf16_t* sW1 = (const bf16_t*)(smem + C2W_OFF_W1);
  const bf16_t* sW2 = (const bf16_t*)(smem + C2W_OFF_W2);
  const bf16_t* sW3 = (const bf16_t*)(smem + C2W_OFF_W3);
  const bf16_t* sW4 = (const bf16_t*)(smem + C2W_OFF_W4);
  float* sb = (float*)(smem + c2w_off_b<PHASE>());
  float* sb1 = sb;
  float* sb2 = sb1 + STEM_C;
  float* sb3 = sb2 + FUS_C;
  float* sb4 = sb3 + ATT_C;
  bf16_t* patch = (bf16_t*)(smem + c2w_off_patch<PHASE>());
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  // ---- one-time LDS fill: weights, biases, BN affines, im2col table
  {
    auto copy_rows = [&](size_t dst, size_t src, int rows, int k, int stride) {  // 16-byte pieces
      const int per = k / 8;
      for (int i = tid; i < rows * per; i += 512) {
        const int rr = i / per, q = i % per;
        *reinterpret_cast<uint4*>(smem + dst + ((size_t)rr * stride + 8 * q) * 2) =
            *reinterpret_cast<const uint4*>(blob + src + ((size_t)rr * k + 8 * q) * 2);
      }
    };
    auto copy_rows_p = [&](size_t dst, const char* base, int rows, int k, int stride) {
      const int per = k / 8;
      for (int i = tid; i < rows * per; i += 512) {
        const int rr = i / per, q = i % per;
        *reinterpret_cast<uint4*>(smem + dst + ((size_t)rr * stride + 8 * q) * 2) =
            *reinterpret_cast<const uint4*>(base + ((size_t)rr * k + 8 * q) * 2);
      }
    };
    if (PHASE == 0)
      copy_rows(C2W_OFF_W1, L.w1s, STEM_C, STEM_K2, C2W_S1);
    else
      copy_rows_p(C2W_OFF_W1, fold + FOLD_W1, STEM_C, STEM_K2, C2W_S1);
    if (PHASE >= 1) {
      if (PHASE == 2)
        copy_rows_p(C2W_OFF_W2, fold + FOLD_W2, FUS_C, STEM_C, C2W_S2);
      else
        copy_rows(C2W_OFF_W2, L.w2, FUS_C, STEM_C, C2W_S2);
    }
    if (PHASE == 2) {  // phase 1 keeps its shifted patch copies there
      copy_rows(C2W_OFF_W3, L.w3, ATT_C, FUS_C, C2W_S3);
      copy_rows(C2W_OFF_W4, L.w4, FUS_C, ATT_C, C2W_S4);
    }
    for (int i = tid; i < STEM_C; i += 512)
      sb1[i] = PHASE == 0 ? ((const float*)(blob + L.b1))[i] : ((const float*)(fold + FOLD_B1))[i];
    for (int i = tid; i < FUS_C; i += 512)
      sb2[i] = PHASE == 2 ? ((const float*)(fold + FOLD_B2))[i] : ((const float*)(blob + L.b2))[i];
    for (int i = tid; i < ATT_C; i += 512) sb3[i] = ((const float*)(blob + L.b3))[i];
    for (int i = tid; i < FUS_C; i += 512) sb4[i] = ((const float*)(blob + L.b4))[i];
    for (int i = tid; i < 3 * C2W_PH * C2W_PWP; i += 512) patch[i] = 0;  // pad columns stay zero
    for (int i = tid; i < STEM_C * (C2W_S1 - STEM_K2); i += 512)  // W1 row pads: never garbage in an MFMA
      ((bf16_t*)(smem + C2W_OFF_W1))[(i / (C2W_S1 - STEM_K2)) * C2W_S1 + STEM_K2 + i % (C2W_S1 - STEM_K2)] = 0;
  }
  // BN statistics (phases 0/1): the layer whose statistics the phase collects runs with its MFMA
  // operands swapped, so its accumulator is [pixel][channel]: lane (r, g) owns channel 16t + r
  // and the pixels {4g .. 4g+3} of each 16-px half.  Running sums stay per lane across tiles (no
  // cross-lane traffic per tile) and the 4 lane groups are combined once, in fixed order, at
  // the end.
  constexpr int NST = PHASE == 0 ? 12 : 8;  // channel tiles whose stats this phase collects
  float ssum[NST], ssq[NST];
#pragma unroll
  for (int i = 0; i < NST; ++i) ssum[i] = ssq[i] = 0.f;
  const int tiles_x = (W + C2W_TW - 1) / C2W_TW, tiles_y = (H + C2W_TH - 1) / C2W_TH;
  const unsigned per = (unsigned)(tiles_x * tiles_y);
  const int ntiles = B * tiles_x * tiles_y;  // < 2^31 (rgbd_ratio_predict checks the shape)
  const long long HW = (long long)H * W;
  // the next tile's depth patch is prefetched into registers while the current one computes
  constexpr int PATCH_N = 3 * C2W_PH * C2W_PW, PATCH_PER = (PATCH_N + 511) / 512;
  float pre[PATCH_PER];
  // Phases 1-2: the loads go through a buffer descriptor, unconditionally; an element outside the
  // image or the patch gets an offset past the descriptor's end, which the hardware returns as
  // zero.  Behind per-element branches (phase 0's form) the compiler waits for each load right
  // where it is issued, so the "prefetch" stalled every phase-1 tile by a memory round trip
  // (3 600 of 18 700 cycles in the stamps); this way nothing reads pre[] before the next tile's
  // staging.  Phase 0 keeps the branches: at four workgroups per CU its waits are hidden, and
  // the other form spilled it past its 128-register budget.
  const long long dbytes = ((long long)(B - 1) * bstride + 3 * HW) * 4;
  const bool dbuf = PHASE >= 1 && dbytes < (1ll << 31);  // 32-bit byte offsets cover the input
  const __amdgpu_buffer_rsrc_t drs = wt_rsrc(depth3, dbuf ? (int)dbytes : 0);
  auto fetch_patch = [&](int t) {
    const TileDec td = tile_dec((unsigned)t, per, (unsigned)tiles_x, C2W_TH, C2W_TW);
#pragma unroll
    for (int k = 0; k < PATCH_PER; ++k) {
      const int i = tid + 512 * k;
      const int c = i / (C2W_PH * C2W_PW), yy = (i / C2W_PW) % C2W_PH, xx = i % C2W_PW;
      const int yv = td.y0 + yy - 3, xv = td.x0 + xx - 3;
      const bool ok = i < PATCH_N && t < ntiles && yv >= 0 && yv < H && xv >= 0 && xv < W;
      if (dbuf) {
        const uint32_t off = ok ? (uint32_t)((td.b * bstride + c * HW + (long long)yv * W + xv) * 4) : 0x80000000u;
        pre[k] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(drs, off, 0, 0));
      } else {
        float v = 0.f;
        if (ok) v = depth3[td.b * bstride + c * HW + (long long)yv * W + xv];
        pre[k] = v;
      }
    }
  };
  // per-lane statistics of a transposed accumulator tile (pixel validity only on ragged tiles)
  auto add_stats = [&](float& sm, float& sq, const f32x4 (&a)[2], bool full, int x0, bool row_ok) {
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float v = a[u][j];
        if (!full) v = (row_ok && x0 + 16 * u + 4 * g + j < W) ? v : 0.f;
        sm += v;
        sq = __builtin_fmaf(v, v, sq);
      }
  };
  fetch_patch(blockIdx.x);
  int tcount = 0;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x, ++tcount) {
    // tiles 8..11 of workgroup 0 (past the start-up: weights landing, every workgroup's first loads)
    unsigned long long* const sts = (STAMPS && blockIdx.x == 0 && tcount >= 8 && tcount < 12) ? g_c2_stamps : nullptr;
    const long long sidx = ((long long)PHASE * 32 + (long long)(tcount - 8) * 8 + wave) * 7;
    if (STAMPS && sts) c2_stamp(sts, sidx + 0);
    const TileDec td = tile_dec((unsigned)tile, per, (unsigned)tiles_x, C2W_TH, C2W_TW);
    const int b = td.b, y0 = td.y0, x0 = td.x0;
    lds_barrier();  // everyone is done with the previous patch
#pragma unroll
    for (int k = 0; k < PATCH_PER; ++k) {
      const int i = tid + 512 * k;
      if (i < PATCH_N) patch[(i / C2W_PW) * C2W_PWP + i % C2W_PW] = f32_to_bf16(pre[k]);
    }
    lds_barrier();
    if constexpr (PHASE == 1) {  // the eight shifted copies, 16 bytes at a time
      // a lane reads copy (col & 7) at elements (col & ~7) .. +7 <= 31: chunks 0..3 of each row
      bf16_t* p8 = (bf16_t*)(smem + C2W_OFF_P8);
      for (int i = tid; i < 8 * 3 * C2W_PH * 4; i += 512) {
        const int j8 = i & 3, row = (i >> 2) % (3 * C2W_PH), k = i / (3 * C2W_PH * 4);
        const int e = 8 * j8 + k;  // first patch column of this chunk (<= 31: five words in the row)
        const uint32_t* wp = reinterpret_cast<const uint32_t*>(patch + row * C2W_PWP + (e & ~1));
        const uint32_t w0 = wp[0], w1 = wp[1], w2 = wp[2], w3 = wp[3], w4 = wp[4];
        const uint32_t sh = (e & 1) * 2;
        *reinterpret_cast<uint4*>(p8 + (k * 3 * C2W_PH + row) * C2W_PWP + 8 * j8) =
            make_uint4(__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh),
                       __builtin_amdgcn_alignbyte(w3, w2, sh), __builtin_amdgcn_alignbyte(w4, w3, sh));
      }
      lds_barrier();
    }
    if (STAMPS && sts) c2_stamp(sts, sidx + 1);
    fetch_patch(tile + gridDim.x);
    if (STAMPS && sts) c2_stamp(sts, sidx + 2);
    const int py = y0 + wave;
    const bool row_ok = py < H;
    const bool full = row_ok && x0 + C2W_TW <= W;  // wave-uniform
    bool pv[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) pv[u] = row_ok && x0 + 16 * u + r < W;
    // ---- stem B operand: K = (c, dy, dx8) groups; lane (r, g) of step s takes group q = 4s + g,
    // i.e. the 8 bf16 patch values (c, row wave+dy, cols 16u+r .. +7): five aligned words from
    // col & ~1 and a byte-align by 2*(col & 1).
    auto stem_b = [&](int s, Frag<bf16_t> (&bf)[2]) {
      const int q = 4 * s + g;
      if constexpr (PHASE == 1) {  // copy (col & 7) = (r & 7) for both halves u, 16 columns apart
        const int qc = q < 21 ? q : 20;
        const int cq = qc / 7, dy = qc - 7 * cq;
        const bf16_t* p8 = (const bf16_t*)(smem + C2W_OFF_P8) + (((r & 7) * 3 + cq) * C2W_PH + wave + dy) * C2W_PWP +
                           (r & 8);
        bf[0].v = *reinterpret_cast<const uint4*>(p8);
        bf[1].v = *reinterpret_cast<const uint4*>(p8 + 16);
        if (q >= 21) {
          bf[0].zero();
          bf[1].zero();
        }
        return;
      }
      const int cq = q / 7, dy = q - 7 * cq;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (q < 21) {
          const int col = 16 * u + r;
          const uint32_t* wp = reinterpret_cast<const uint32_t*>(patch + (cq * C2W_PH + wave + dy) * C2W_PWP + (col & ~1));
          const uint32_t w0 = wp[0], w1 = wp[1], w2 = wp[2], w3 = wp[3], w4 = wp[4];
          const uint32_t sh = (col & 1) * 2;
          bf[u].v = make_uint4(__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh),
                               __builtin_amdgcn_alignbyte(w3, w2, sh), __builtin_amdgcn_alignbyte(w4, w3, sh));
        } else {
          bf[u].zero();
        }
      }
    };
    // Zero K blocks of the 3x3 / 5x5 filters embedded in the 7x7 window are skipped (channel
    // groups t < 4 use steps {0,1,2,4}, t < 8 steps 0..4, t >= 8 all six); groups 21..23 of
    // step 5 lie past the 168 packed columns.  Accumulators start at the bias.
    auto stem_w = [&](int t, int s) {
      Frag<bf16_t> af;
      af.v = *reinterpret_cast<const uint4*>(sW1 + (16 * t + r) * C2W_S1 + 32 * s + 8 * g);
      if (s == 5) af.select(g == 0);
      return af;
    };
    auto stem_live = [](int t, int s) { return !((t < 4 && (s == 3 || s == 5)) || (t >= 4 && t < 8 && s == 5)); };
    if constexpr (PHASE == 0) {
      // statistics only: channel group outermost with the operands swapped (accumulator
      // [pixel][channel]), all six B fragments built once, two accumulators live at a time
      Frag<bf16_t> bfr[6][2];
#pragma unroll
      for (int s = 0; s < 6; ++s) stem_b(s, bfr[s]);
#pragma unroll
      for (int t = 0; t < 12; ++t) {
        const float bb = sb1[16 * t + r];
        f32x4 a1[2] = {f32x4{bb, bb, bb, bb}, f32x4{bb, bb, bb, bb}};
#pragma unroll
        for (int s = 0; s < 6; ++s) {
          if (!stem_live(t, s)) continue;
          const Frag<bf16_t> af = stem_w(t, s);
          mma(a1[0], bfr[s][0], af);
          mma(a1[1], bfr[s][1], af);
        }
        add_stats(ssum[t], ssq[t], a1, full, x0, row_ok);
      }
      if (STAMPS && sts) c2_stamp(sts, sidx + 3);
      continue;
    }
    // phases 1, 2: K step outermost (one B fragment pair live), all 12 channel groups accumulate
    f32x4 a1[12][2];
#pragma unroll
    for (int t = 0; t < 12; ++t) {
      const float4 bb = *reinterpret_cast<const float4*>(sb1 + 16 * t + 4 * g);
      a1[t][0] = a1[t][1] = f32x4{bb.x, bb.y, bb.z, bb.w};
    }
    if constexpr (PHASE == 1) {
      // one K step of patch fragments in flight ahead of the MFMAs that use the current one
      // (the scheduling fences keep the compiler from hoisting more steps: register budget)
      Frag<bf16_t> bcur[2], bnxt[2];
      stem_b(0, bcur);
#pragma unroll
      for (int s = 0; s < 6; ++s) {
        if (s < 5) stem_b(s + 1, bnxt);
#pragma unroll
        for (int t = 0; t < 12; ++t) {
          if (!stem_live(t, s)) continue;
          const Frag<bf16_t> af = stem_w(t, s);
          mma(a1[t][0], af, bcur[0]);
          mma(a1[t][1], af, bcur[1]);
        }
        __builtin_amdgcn_sched_barrier(0);
        bcur[0] = bnxt[0];
        bcur[1] = bnxt[1];
      }
    } else {
#pragma unroll
      for (int s = 0; s < 6; ++s) {
        Frag<bf16_t> bfr[2];
        stem_b(s, bfr);
#pragma unroll
        for (int t = 0; t < 12; ++t) {
          if (!stem_live(t, s)) continue;
          const Frag<bf16_t> af = stem_w(t, s);
          mma(a1[t][0], af, bfr[0]);
          mma(a1[t][1], af, bfr[1]);
        }
      }
    }
    if (STAMPS && sts) c2_stamp(sts, sidx + 3);
    Frag<bf16_t> f1[6][2];
#pragma unroll
    for (int s = 0; s < 6; ++s)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        float vv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) vv[e] = fmaxf(a1[2 * s + (e >> 2)][u][e & 3], 0.f);  // BN1 folded into W1
        f1[s][u].from8(vv);
      }
    if (STAMPS && sts) c2_stamp(sts, sidx + 4);
    // ---- fusion (phase 1: operands swapped for the statistics)
    f32x4 a2[8][2];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      if constexpr (PHASE == 1) {
        const float bb = sb2[16 * t + r];
        a2[t][0] = a2[t][1] = f32x4{bb, bb, bb, bb};
      } else {
        const float4 bb = *reinterpret_cast<const float4*>(sb2 + 16 * t + 4 * g);
        a2[t][0] = a2[t][1] = f32x4{bb.x, bb.y, bb.z, bb.w};
      }
#pragma unroll
      for (int s = 0; s < 6; ++s) {
        Frag<bf16_t> af;
        af.v = *reinterpret_cast<const uint4*>(sW2 + (16 * t + r) * C2W_S2 + 32 * s + 8 * g);
        if constexpr (PHASE == 1) {
          mma(a2[t][0], f1[s][0], af);
          mma(a2[t][1], f1[s][1], af);
        } else {
          mma(a2[t][0], af, f1[s][0]);
          mma(a2[t][1], af, f1[s][1]);
        }
      }
    }
    if (STAMPS && sts) c2_stamp(sts, sidx + 5);
    if constexpr (PHASE == 1) {
#pragma unroll
      for (int t = 0; t < 8; ++t) add_stats(ssum[t], ssq[t], a2[t], full, x0, row_ok);
      if (att) {  // raw fusion output for k_rp_gate: [tile][wave][t][lane][u][4 px], 1 KiB per store
        bf16_t* ft = att + (((long long)tile * 8 + wave) * 16) * 256;
#pragma unroll
        for (int t = 0; t < 8; ++t)
          *reinterpret_cast<uint4*>(ft + (t * 64 + lane) * 8) =
              make_uint4(pack_bf16x2(a2[t][0][0], a2[t][0][1]), pack_bf16x2(a2[t][0][2], a2[t][0][3]),
                         pack_bf16x2(a2[t][1][0], a2[t][1][1]), pack_bf16x2(a2[t][1][2], a2[t][1][3]));
      }
      if (STAMPS && sts) c2_stamp(sts, sidx + 6);
      continue;
    }
    if constexpr (PHASE == 2) {
#pragma unroll
      for (int t = 0; t < 8; ++t)  // BN2 folded into W2
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          a2[t][0][j] = fmaxf(a2[t][0][j], 0.f);
          a2[t][1][j] = fmaxf(a2[t][1][j], 0.f);
        }
      Frag<bf16_t> f2[4][2];
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          float vv[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) vv[e] = a2[2 * s + (e >> 2)][u][e & 3];
          f2[s][u].from8(vv);
        }
      f32x4 a3[4][2];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float4 bb = *reinterpret_cast<const float4*>(sb3 + 16 * t + 4 * g);
        a3[t][0] = a3[t][1] = f32x4{bb.x, bb.y, bb.z, bb.w};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          Frag<bf16_t> af;
          af.v = *reinterpret_cast<const uint4*>(sW3 + (16 * t + r) * C2W_S3 + 32 * s + 8 * g);
          mma(a3[t][0], af, f2[s][0]);
          mma(a3[t][1], af, f2[s][1]);
        }
      }
      Frag<bf16_t> f3[2][2];
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          float vv[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) vv[e] = fmaxf(a3[2 * s + (e >> 2)][u][e & 3], 0.f);
          f3[s][u].from8(vv);
        }
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const float4 bb = *reinterpret_cast<const float4*>(sb4 + 16 * t + 4 * g);
        f32x4 a4[2] = {f32x4{bb.x, bb.y, bb.z, bb.w}, f32x4{bb.x, bb.y, bb.z, bb.w}};
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          Frag<bf16_t> af;
          af.v = *reinterpret_cast<const uint4*>(sW4 + (16 * t + r) * C2W_S4 + 32 * s + 8 * g);
          mma(a4[0], af, f3[s][0]);
          mma(a4[1], af, f3[s][1]);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          if (!pv[u]) continue;
          float o[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = a2[t][u][j] * sigmoid_fast(a4[u][j]);
          // conv5 v4's padded channel-quarter-major planes (c4_att_idx)
          *reinterpret_cast<uint2*>(att + c4_att_idx(b, t >> 1, py, x0 + 16 * u + r, H, W) + 16 * (t & 1) + 4 * g) =
              make_uint2(pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]));
        }
      }
    }
  }
  if constexpr (PHASE < 2) {
    // lanes r, r+16, r+32, r+48 hold channel 16t + r: combine in fixed order, one slab row per wave
    const long long row = (long long)blockIdx.x * 8 + wave;
    constexpr int NC = PHASE == 0 ? STEM_C : FUS_C;
#pragma unroll
    for (int t = 0; t < NST; ++t) {
      float a = ssum[t], q = ssq[t];
      a += __shfl_xor(a, 16);
      q += __shfl_xor(q, 16);
      a += __shfl_xor(a, 32);
      q += __shfl_xor(q, 32);
      if (g == 0) {
        // phase 1: channel-major (k_bn_affine cm = 1); phase 0: row-major (k_bn_affine_stem)
        const long long e = PHASE == 1 ? (long long)(16 * t + r) * (gridDim.x * 8) + row : row * NC + 16 * t + r;
        slab[e * 2 + 0] = a;
        slab[e * 2 + 1] = q;
      }
    }
  }
}

// phase PH's kernel over its persistent grid; the diagnostic build's stamped instantiation when
// rgbd_debug_chain_stamps has armed it (phases 0 and 1)
template <int PH>
int chain_launch(const float* depth3, long long bstride, int B, int H, int W, const char* blob, const Layout& L,
                 const float2* aff1, const float2* aff2, const char* fold, float* slab, bf16_t* att, hipStream_t s) {
  static const hipError_t attr = hipFuncSetAttribute((const void*)k_rp_chain_v2<PH>,
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)c2w_smem<PH>());
  if (attr != hipSuccess) return (int)attr;
  const int grid = chain_grid_v2(B, H, W, PH);
#ifdef RGBD_DIAG
  if constexpr (PH < 2) {
    if (c2_stamps_on) {
      static const hipError_t sattr = hipFuncSetAttribute(
          (const void*)k_rp_chain_v2<PH, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c2w_smem<PH>());
      (void)sattr;
      k_rp_chain_v2<PH, true><<<grid, 512, c2w_smem<PH>(), s>>>(depth3, bstride, B, H, W, blob, L, aff1, aff2, fold,
                                                               slab, att);
      return RGBD_OK;
    }
  }
#endif
  k_rp_chain_v2<PH><<<grid, 512, c2w_smem<PH>(), s>>>(depth3, bstride, B, H, W, blob, L, aff1, aff2, fold, slab, att);
  return RGBD_OK;
}

}  // namespace

namespace rgbd::rp {

// one 512-thread workgroup per CU (LDS-resident weights); phase 0 two
int chain_grid_v2(int B, int H, int W, int phase) {
  const long long nt = (long long)B * ((W + C2W_TW - 1) / C2W_TW) * ((H + C2W_TH - 1) / C2W_TH);
  return (int)std::min<long long>(nt, phase == 0 ? 512 : 256);
}

// BN1 -> W1', b1' (which = 1) or BN2 -> W2', b2' (which = 2)
int fold_bn(const char* blob, const Layout& L, const float2* aff, int which, char* fold, hipStream_t s) {
  k_rp_fold<<<which == 1 ? STEM_C : FUS_C, 256, 0, s>>>(blob, L, aff, which, fold);
  return RGBD_OK;
}

// phase 0: stem statistics -> slab; 1: fusion statistics -> slab (+ the raw fusion output -> att,
// when given, for k_rp_gate); 2: the gated attention features -> att
int chain_v2(int phase, const float* depth3, long long bstride, int B, int H, int W, const char* blob, const Layout& L,
             const float2* aff1, const float2* aff2, const char* fold, float* slab, bf16_t* att, hipStream_t s) {
  if (phase == 0) return chain_launch<0>(depth3, bstride, B, H, W, blob, L, aff1, aff2, fold, slab, att, s);
  if (phase == 1) return chain_launch<1>(depth3, bstride, B, H, W, blob, L, aff1, aff2, fold, slab, att, s);
  TimerScope ts("rp_chain", s);
  return chain_launch<2>(depth3, bstride, B, H, W, blob, L, aff1, aff2, fold, slab, att, s);
}

}  // namespace rgbd::rp

#ifdef RGBD_DIAG
extern "C" int rgbd_debug_chain_stamps(void* buf) {
  unsigned long long* p = (unsigned long long*)buf;
  const hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(g_c2_stamps), &p, sizeof(p));
  if (e != hipSuccess) return (int)e;
  c2_stamps_on = p != nullptr;
  return RGBD_OK;
}
#endif
