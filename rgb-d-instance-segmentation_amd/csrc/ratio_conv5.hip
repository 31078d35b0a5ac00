// K4 stage file: the bf16 gate (k_rp_gate) and conv5 3x3 128->256 (k_rp_conv5_v4) with its input
// padding (k_c4_pad_zero) and its BN + ReLU + pool kernels (k_rp_bn_relu_pool_v4_tiles / _frag,
// k_rp_pool_finish_v4).  Gate and conv5 sit together: they are the pair DESIGN section 9 wants
// fused into one persistent kernel.  Overview: ratio.hip.
#include "ratio_common.hpp"

using namespace rgbd;
using namespace rgbd::rp;

namespace {

// ---- train mode, bf16: the chain's last stage from phase 1's stored fusion output.
// Phase 1 has to run the stem + fusion for the BN2 statistics anyway; storing its raw fusion
// output (fragment-native, 256 B/px) lets this kernel skip the stem + fusion recompute that
// phase 2 would do (111 k FLOP/px): per 8x32-px tile a wave owns one pixel row, reads its 8 KB,
// applies BN2 + ReLU, transposes through a wave-private LDS image [32 px][128 ch], and runs the
// attention 1x1s (128->64->128, LDS-resident weights) and the sigmoid gate; HBM-bound
// (512 B/px).  The eval path (no statistics pass) keeps phase 2.
constexpr int GT_S = FUS_C + 8;  // image row: 128 channels + 8 pad (272 B, conflict-free b64 reads)
constexpr size_t GT_OFF_W3 = 0;
constexpr size_t GT_OFF_W4 = GT_OFF_W3 + (size_t)ATT_C * C2W_S3 * 2;
constexpr size_t GT_OFF_B = GT_OFF_W4 + (size_t)FUS_C * C2W_S4 * 2;  // b3[64], b4[128], aff2[128]
constexpr size_t GT_OFF_IMG = GT_OFF_B + (size_t)(ATT_C + FUS_C + 2 * FUS_C) * 4;
constexpr size_t GT_SMEM = GT_OFF_IMG + (size_t)8 * C2W_TW * GT_S * 2;
static_assert(GT_SMEM <= 163840, "gate LDS budget");

__global__ __launch_bounds__(512) void k_rp_gate(const bf16_t* __restrict__ fus, int B, int H, int W,
                                                 const char* __restrict__ blob, Layout L,
                                                 const float2* __restrict__ aff2, bf16_t* __restrict__ att) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const bf16_t* sW3 = (const bf16_t*)(smem + GT_OFF_W3);
  const bf16_t* sW4 = (const bf16_t*)(smem + GT_OFF_W4);
  float* sb3 = (float*)(smem + GT_OFF_B);
  float* sb4 = sb3 + ATT_C;
  float2* saff = (float2*)(sb4 + FUS_C);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  bf16_t* img = (bf16_t*)(smem + GT_OFF_IMG) + (size_t)wave * C2W_TW * GT_S;
  {
    auto copy_rows = [&](size_t dst, size_t src, int rows, int k, int stride) {
      const int per = k / 8;
      for (int i = tid; i < rows * per; i += 512) {
        const int rr = i / per, q = i % per;
        *reinterpret_cast<uint4*>(smem + dst + ((size_t)rr * stride + 8 * q) * 2) =
            *reinterpret_cast<const uint4*>(blob + src + ((size_t)rr * k + 8 * q) * 2);
      }
    };
    copy_rows(GT_OFF_W3, L.w3, ATT_C, FUS_C, C2W_S3);
    copy_rows(GT_OFF_W4, L.w4, FUS_C, ATT_C, C2W_S4);
    for (int i = tid; i < ATT_C; i += 512) sb3[i] = ((const float*)(blob + L.b3))[i];
    for (int i = tid; i < FUS_C; i += 512) {
      sb4[i] = ((const float*)(blob + L.b4))[i];
      saff[i] = aff2[i];
    }
  }
  __syncthreads();
  const int tiles_x = (W + C2W_TW - 1) / C2W_TW, tiles_y = (H + C2W_TH - 1) / C2W_TH;
  const unsigned per = (unsigned)(tiles_x * tiles_y);
  const int ntiles = B * tiles_x * tiles_y;
  // this wave's raw fusion output of a tile ([t][lane][u][4 px]): lane (r, g) has channel 16t + r,
  // pixels 16u + 4g + j;
  // the next tile's 8 KB are loaded while the current one computes
  uint2 nxt[8][2];
  auto fetch = [&](int tl) {
    if (tl >= ntiles) return;
    const int tp = ntiles - 1 - tl;  // physical tile: last-to-first (see conv5 v4's tile order)
    const bf16_t* ft = fus + (((long long)tp * 8 + wave) * 16) * 256;
#pragma unroll
    for (int t = 0; t < 8; ++t) {  // read once: non-temporal, 16 B per lane (1 KiB per wave load)
      const u32x4 q = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(ft + (t * 64 + lane) * 8));
      nxt[t][0] = make_uint2(q[0], q[1]);
      nxt[t][1] = make_uint2(q[2], q[3]);
    }
  };
  // (one tile ahead: two and three tiles ahead measured the same, 0.252-0.258 ms, round 6)
  fetch(blockIdx.x);
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const TileDec td = tile_dec((unsigned)(ntiles - 1 - tile), per, (unsigned)tiles_x, C2W_TH, C2W_TW);
    const int b = td.b, y0 = td.y0, x0 = td.x0;
    const int py = y0 + wave;
    uint2 raw[8][2];
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
      for (int u = 0; u < 2; ++u) raw[t][u] = nxt[t][u];
    fetch(tile + gridDim.x);
    if (py >= H) continue;  // wave-uniform; nothing below synchronises across waves
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // previous tile's image reads are done
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int c = 16 * t + r;
      const float2 a = saff[c];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const uint32_t w01 = raw[t][u].x, w23 = raw[t][u].y;
        const float v[4] = {__uint_as_float(w01 << 16), __uint_as_float(w01 & 0xffff0000u),
                            __uint_as_float(w23 << 16), __uint_as_float(w23 & 0xffff0000u)};
#pragma unroll
        for (int j = 0; j < 4; ++j)
          img[(16 * u + 4 * g + j) * GT_S + c] = f32_to_bf16(fmaxf(__builtin_fmaf(v[j], a.x, a.y), 0.f));  // BN2 + ReLU
      }
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    // ---- W3 B operand in the chain's K order: element e of chunk s = channel 32s + 16(e>>2) + 4g + (e&3)
    Frag<bf16_t> f2[4][2];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const bf16_t* row = img + (16 * u + r) * GT_S + 32 * s + 4 * g;
        const uint2 lo = *reinterpret_cast<const uint2*>(row), hi = *reinterpret_cast<const uint2*>(row + 16);
        f2[s][u].v = make_uint4(lo.x, lo.y, hi.x, hi.y);
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
        // the gated value replaces the activation it came from (same lane, same 8 bytes)
        uint2* cell = reinterpret_cast<uint2*>(img + (16 * u + r) * GT_S + 16 * t + 4 * g);
        const uint2 act = *cell;
        const float av[4] = {__uint_as_float(act.x << 16), __uint_as_float(act.x & 0xffff0000u),
                             __uint_as_float(act.y << 16), __uint_as_float(act.y & 0xffff0000u)};
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = av[j] * sigmoid_fast(a4[u][j]);
        *cell = make_uint2(pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3]));
      }
    }
    // store into conv5 v4's padded channel-quarter-major planes (c4_att_idx) of the wave's 32 pixels
    // from the image: per store instruction one quarter of 16 consecutive pixels (1 KB contiguous)
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int qt = k >> 1, pr = 16 * (k & 1) + (lane >> 2), q = lane & 3;
      if (x0 + pr < W)
        *reinterpret_cast<uint4*>(att + c4_att_idx(b, qt, py, x0 + pr, H, W) + 8 * q) =
            *reinterpret_cast<const uint4*>(img + pr * GT_S + 32 * qt + 8 * q);
    }
  }
}

// ---- conv5 v4 (bf16): a work item is a 16x32-pixel tile x one 128-channel half of the output
// (512 px x 128 ch; the two halves of a tile run at the same time on two workgroups of one XCD,
// so the second one's input copies hit the L2 the first one filled).  8 waves, wave w = tile
// rows 2w, 2w+1 (64 px) x all 128 channels = 4x8 MFMA 16x16x32 tiles (the v3 wave tile).  K is
// walked in 12 steps of (input-channel quarter qt, kernel row ky), each step the 3 taps kx of
// that row over the quarter's 32 channels (K 96: 96 MFMAs per wave between two barriers).
// Against v3's 256 px x 256 ch items this halves the weight copies per FLOP (the weights of a
// step serve 512 pixels) at a slightly larger input share: 445 KB of LDS-DMA per item instead of
// 2 x 332 KB for the same FLOPs (-33 %), ~4.6 one-KiB pieces per wave and step instead of 9
// per loader wave.
// LDS: two input slots (quarter qt in slot qt & 1: the whole 18x34 halo x 32 channels, 64-byte
// rows, 16-byte chunk c at slot c ^ ((row >> 1) & 2): ds_read_b128 conflict-free for 16
// consecutive rows from any start row), two weight buffers of one step ([kx][n][32 ch], the same
// swizzle, pre-applied in the blob so a step is one linear 24 KiB copy).
// Pipeline: in step st waves 0-3 issue the weights of step st+1 (the next item's step 0 after
// the last: a workgroup always owns the same channel half) before their MFMAs; waves 4-7 issue
// a third of the next quarter's input (the next item's quarter 0 during quarter 3) after their
// first 32 MFMAs; every wave waits for its own copies, then the step's one barrier.  Every copy
// is an LDS-DMA from a wave-uniform base (scalar registers) + a 32-bit lane offset; the tile
// origins are computed once per item.
// Fragments: per kx group a wave reads its 4 A fragments and B columns 0-3, then issues the
// MFMAs column by column (nj outer, mi inner) and reads column nj + 4 into column nj's
// registers right behind that column's MFMAs: 32 fragment registers, the second half of the B
// reads under MFMAs.  Every A address of a step is one of eight per-lane bases + an immediate.
// Reading the next group's or the next step's fragments ahead (a three-step weight ring for the
// latter) measured no faster / slower: DESIGN 5.10.1.
// MODE 0 (train): y stored fragment-native per item [item = 2 tile + half][wave][mi][np][lane][8]
//   (1 KiB contiguous per store instruction) and the BN statistics of the float32 conv outputs
//   kept in registers across items -> slab[256][workgroup][2] (the other half's entries zero).
// MODE 1 (eval, H % 4 == 0, W % 64 == 0, H >= 64, W >= 128: every 16-px fragment row lies in one
//   AdaptiveAvgPool(4) bin): BN (running statistics, `aff`) + ReLU of the bf16-rounded outputs
//   summed per pool bin in the epilogue -> out[item][4 bin slots][128]; no y.
// MODE 2 (eval, other shapes): y only.
// Tile order: every kernel of the chain -> gate -> conv5 -> pool sequence reads first what the
// previous one wrote last (still in the Infinity Cache): the chain writes its tiles first to last,
// the gate walks them last to first, conv5 first to last, the pool the images last to first
// (round 5: profiles/r05_v2/ab_w.txt, ab_zk.txt).
constexpr int C4_NPIX = (C4_TH + 2) * C4_PW;  // 612 halo pixels
constexpr int C4_APIECES = 39;                // 624 rows of 64 B, 16 rows per 1 KiB piece
constexpr int C4_A_BYTES = C4_APIECES * 1024;
constexpr int C4_STEPS = 12;
constexpr int C4_B_BYTES = 3 * 128 * 64;  // one step: [kx][n][32 ch]
constexpr int C4_B_OFF = 2 * C4_A_BYTES;
constexpr int C4_RED_OFF = C4_B_OFF + 2 * C4_B_BYTES;
constexpr int C4_RED_BYTES = 8 * 4 * 128 * 4;  // MODE 1: per (wave, mi) bin sums of 128 channels
constexpr int C4_PAR_OFF = C4_RED_OFF + C4_RED_BYTES;
constexpr size_t C4_SMEM = C4_PAR_OFF + 128 * 4 + 128 * 8 + 32 * 4;  // bias, BN affine, bin slots
static_assert(C4_SMEM <= 163840, "conv5 v4 LDS budget");
static_assert(C4_APIECES * 16 >= C4_NPIX && C4_APIECES % 3 == 0, "conv5 v4 input pieces");
constexpr int C4_AK = (C4_APIECES + 3) / 4;  // input pieces per copying wave and quarter
static_assert(2 * C4_A_BYTES >= 8 * 128 * 2 * 4, "conv5 v4 statistics scratch");

__device__ __forceinline__ uint32_t c4_off(int row, int chunk) { return row * 64 + 16 * (chunk ^ ((row >> 1) & 2)); }

// LDS-DMA of 16 bytes per lane from a wave-uniform base + a 32-bit per-lane offset (no 64-bit
// per-lane address arithmetic, no address register pair per piece)
__device__ __forceinline__ void c4_dma(const void* sbase, uint32_t voff, uint32_t lds_base) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(voff), "s"(sbase), "s"(lds_base)
               : "memory");
}

struct C4Tile {
  int b, y0, x0;
};
__device__ __forceinline__ C4Tile c4_tile(long long t, int tiles_x, int tiles_y) {
  C4Tile o;
  const long long per = (long long)tiles_x * tiles_y;
  o.b = (int)(t / per);
  const int rem = (int)(t % per);
  o.y0 = (rem / tiles_x) * C4_TH;
  o.x0 = (rem % tiles_x) * C4_TW;
  return o;
}

// C4_NODMA (experiment builds only, -DC4_NODMA=bits; results wrong, timing only): bit 0 drops the
// in-loop weight copies, bit 1 the in-loop input copies, bit 2 the step barrier, bit 3 the
// fragment reads (constant operands)
#ifndef C4_NODMA
#define C4_NODMA 0
#endif


// Stamps (the diagnostic build, RGBD_DIAG: rgbd_debug_conv5_stamps): workgroup 0 records, per step
// and wave of its first two items, s_memtime at the step top, after the weight-copy issue, after
// the first kx group (+ the input-copy issue), after the last MFMAs, after the closing wait +
// barrier: stamps[((item * 12 + step) * 8 + wave) * 5 + k].  The product build has no stamp code.
#if defined(RGBD_DIAG) && !defined(C4_STAMPS)
#define C4_STAMPS
#endif
#ifdef C4_STAMPS
__device__ unsigned long long* g_c4_stamps = nullptr;
__device__ __forceinline__ void c4_stamp(unsigned long long* st, long long idx) {
  __builtin_amdgcn_sched_barrier(0);
  const unsigned long long t = __builtin_amdgcn_s_memtime();
  if ((threadIdx.x & 63) == 0) st[idx] = t;
  __builtin_amdgcn_sched_barrier(0);
}
#define C4_STAMP(k) \
  if (sts) c4_stamp(sts, (((long long)tcount * C4_STEPS + st) * 8 + wave) * 5 + (k))
#else
#define C4_STAMP(k)
#endif
template <int MODE>
__global__ __launch_bounds__(512) void k_rp_conv5_v4(const bf16_t* __restrict__ x, int B, int H, int W,
                                                     const char* __restrict__ blob, Layout L,
                                                     const float2* __restrict__ aff, bf16_t* __restrict__ y,
                                                     float* __restrict__ out, int xcd_pairs) {
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;
  const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
  // workgroups b and b + 8 (one XCD under round-robin placement: speed only) share the tiles
  int pair, nh;
  if (xcd_pairs) {
    nh = (blockIdx.x >> 3) & 1;
    pair = (blockIdx.x & 7) | ((blockIdx.x >> 4) << 3);
  } else {
    nh = blockIdx.x & 1;
    pair = blockIdx.x >> 1;
  }
  const int npairs = gridDim.x >> 1;
  const char* w5q = blob + L.w5q + (size_t)nh * C4_STEPS * C4_B_BYTES;
  float* sbias = (float*)(smem + C4_PAR_OFF);
  float2* saff = (float2*)(smem + C4_PAR_OFF + 512);
  int* sslot = (int*)(smem + C4_PAR_OFF + 512 + 1024);
  for (int i = tid; i < 128; i += 512) {
    sbias[i] = ((const float*)(blob + L.b5))[nh * 128 + i];
    if constexpr (MODE == 1) saff[i] = aff[nh * 128 + i];
  }
  const int tiles_x = (W + C4_TW - 1) / C4_TW, tiles_y = (H + C4_TH - 1) / C4_TH;
  const long long ntiles = (long long)B * tiles_x * tiles_y;

  // input piece j (rows 16j .. 16j+15 of the halo image) of quarter qt of tile t into slot sl:
  // the copying waves (4-7) own pieces j = w4 + 4k (k < 10); a lane's source offset from the
  // tile's padded origin depends on the piece and the plane width only, so it is computed once
  const int PW = c4_pw(W);
  const long long plane = (long long)c4_ph(H) * PW * 32;  // elements
  uint32_t aoff[C4_AK];
#pragma unroll
  for (int k = 0; k < C4_AK; ++k) {
    const int row = 16 * ((wave & 3) + 4 * k) + (lane >> 2), q = lane & 3;
    const int hy = row / C4_PW, hx = row - hy * C4_PW;
    aoff[k] = row < C4_NPIX ? (uint32_t)((hy * PW + hx) * 64 + 16 * (q ^ ((row >> 1) & 2))) : 0u;
  }
  // xt: the tile's padded origin in quarter plane 0 of its image
  auto issue_a = [&](const bf16_t* xt, int qt, int sl, int k) {
    c4_dma(xt + qt * plane, aoff[k], lds0 + sl * C4_A_BYTES + ((wave & 3) + 4 * k) * 1024);
  };
  auto tile_origin = [&](const C4Tile& t) { return x + (long long)t.b * 4 * plane + ((long long)t.y0 * PW + t.x0) * 32; };
  // weight pieces k0..k1-1 (of 24) of step st into buffer st & 1
  auto issue_b = [&](int st, int k0, int k1) {
    const char* src = w5q + (size_t)st * C4_B_BYTES;
    const uint32_t dst = lds0 + C4_B_OFF + (st & 1) * C4_B_BYTES;
    for (int k = k0; k < k1; ++k) c4_dma(src + 1024 * k, 16 * lane, dst + 1024 * k);
  };
  const bool loader = wave < 4;

  f32x2 ssum[8], ssq[8];
#pragma unroll
  for (int nj = 0; nj < 8; ++nj) ssum[nj] = ssq[nj] = f32x2{0.f, 0.f};
  const int rh = H >> 2, rw = W >> 2;  // MODE 1: pool bin size

#ifndef C4_NOPRIO
  // the copying waves' partners compute first (static priority; loaders at equal priority
  // measured +20 %, loaders at priority +12 %)
  if (wave >= 4) __builtin_amdgcn_s_setprio(1);
#endif
  long long tile = pair;
  if (tile < ntiles) {  // prologue: quarter 0 (waves 4-7) + the weights of step 0
    const C4Tile t = c4_tile(tile, tiles_x, tiles_y);
    if (!loader) {
#pragma unroll
      for (int k = 0; k < C4_AK; ++k)
        if ((wave & 3) + 4 * k < C4_APIECES) issue_a(tile_origin(t), 0, 0, k);
    }
    issue_b(0, 3 * wave, 3 * wave + 3);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  // Fragment addresses.  A row mi of tap (ky, kx) is halo pixel p = P + c, P = 68 wave + r + C4_PW ky
  // per lane and step, c = (mi >> 1) * C4_PW + (mi & 1) * 16 + kx a constant; c4_off(p, g) = 64 p +
  // (16 g ^ 32 bit2(p)) and bit2(P + c) = bit2(P + (c & 7)), so eight per-lane bases xa[c & 7],
  // computed at the step top, and the constant 64 c as the read's immediate offset give every
  // address of the step.
  // B column nj of tap kx is row 128 kx + 16 nj + r, whose swizzle depends on r alone: one base.
  uint32_t xa[8];
  const uint32_t xb = C4_B_OFF + c4_off(r, g);
  auto rd_a = [&](int kx, int mi) {
    if constexpr (C4_NODMA & 8) return make_uint4(lane, kx, 0, mi);
    const int c = (mi >> 1) * C4_PW + (mi & 1) * 16 + kx;
    return *reinterpret_cast<const uint4*>(smem + xa[c & 7] + 64 * c);
  };
  auto rd_b = [&](uint32_t bo, int kx, int nj) {  // bo = xb + the weight buffer's offset
    if constexpr (C4_NODMA & 8) return make_uint4(nj, lane, kx, 0);
    return *reinterpret_cast<const uint4*>(smem + bo + (kx * 128 + 16 * nj) * 64);
  };
  Frag<bf16_t> fa[4], fb[4];
#ifdef C4_STAMPS
  int tcount = 0;
#endif
  for (; tile < ntiles; tile += npairs) {
#ifdef C4_STAMPS
    unsigned long long* const sts = (blockIdx.x == 0 && tcount < 2) ? g_c4_stamps : nullptr;
#endif
    const C4Tile t = c4_tile(tile, tiles_x, tiles_y);
    const long long ntile = tile + npairs;
    const bool has_next = ntile < ntiles;
    const C4Tile tn = c4_tile(has_next ? ntile : tile, tiles_x, tiles_y);
    // the origins of this tile and the next one, once per item (selecting between the tiles at
    // each copy repeated the tile decomposition's divisions there)
    const bf16_t *xt = tile_origin(t), *xn = tile_origin(tn);
    f32x4 acc[4][8];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int nj = 0; nj < 8; ++nj) acc[mi][nj] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
    for (int st = 0; st < C4_STEPS; ++st) {
      const int qt = st / 3, ky = st - 3 * qt;
      const int qn = qt + 1;  // the quarter copied during this one (4: the next item's quarter 0)
      const bool a_go = !(C4_NODMA & 2) && !loader && (qn < 4 || has_next);
      C4_STAMP(0);
      if (!(C4_NODMA & 1) && loader && (st + 1 < C4_STEPS || has_next))
        issue_b(st + 1 < C4_STEPS ? st + 1 : 0, 6 * wave, 6 * wave + 6);
      C4_STAMP(1);
      const uint32_t sb = xb + (st & 1) * C4_B_BYTES;
#pragma unroll
      for (int k = 0; k < 8; ++k)
        xa[k] = (qt & 1) * C4_A_BYTES + c4_off(68 * wave + r + C4_PW * ky + k, g) - 64 * k;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        // The group's 4 A fragments and its first 4 B fragments; column nj's B registers take
        // column nj + 4 as soon as its four MFMAs are issued, so the second half of the B reads
        // runs under MFMAs.  Each accumulator gets one MFMA per group: the order inside a group
        // is free, the K order (quarter, ky, kx) of every accumulator is unchanged.
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) fa[mi].v = rd_a(kx, mi);
#pragma unroll
        for (int nj = 0; nj < 4; ++nj) fb[nj].v = rd_b(sb, kx, nj);
#pragma unroll
        for (int nj = 0; nj < 8; ++nj) {
#pragma unroll
          for (int mi = 0; mi < 4; ++mi) mma(acc[mi][nj], fa[mi], fb[nj & 3]);
          __builtin_amdgcn_sched_barrier(0);  // the read stays between this column's MFMAs and the next one's
          if (nj < 4) fb[nj].v = rd_b(sb, kx, nj + 4);
          __builtin_amdgcn_sched_barrier(0);
        }
        if (kx == 0 && a_go) {  // this step's 13 pieces [13 ky, 13 ky + 13) of the next quarter
#pragma unroll
          for (int k = 0; k < C4_AK; ++k) {
            const int j = (wave & 3) + 4 * k;
            if (j >= 13 * ky && j < 13 * ky + 13 && j < C4_APIECES) issue_a(qn < 4 ? xt : xn, qn & 3, qn & 1, k);
          }
        }
        if (kx == 0) C4_STAMP(2);
      }
      C4_STAMP(3);
      if constexpr (C4_NODMA & 4)
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      else
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
      C4_STAMP(4);
    }
#ifdef C4_STAMPS
    ++tcount;
#endif

    // ---- epilogue
    const long long item = 2 * tile + nh;
    if constexpr (MODE != 1) {
      bf16_t* yt = y + ((item * 8 + wave) * 16) * 512;  // [mi][np][lane][8]
      const bool interior = t.y0 + C4_TH <= H && t.x0 + C4_TW <= W;
#pragma unroll
      for (int np = 0; np < 4; ++np) {
        const float b0 = sbias[32 * np + r], b1 = sbias[32 * np + 16 + r];
        if (interior) {
          const f32x2 bb0 = {b0, b0}, bb1 = {b1, b1};
#pragma unroll
          for (int mi = 0; mi < 4; ++mi) {
            const f32x4 v = acc[mi][2 * np], w = acc[mi][2 * np + 1];
            const f32x2 a0 = f32x2{v[0], v[1]} + bb0, a1 = f32x2{v[2], v[3]} + bb0;
            const f32x2 c0 = f32x2{w[0], w[1]} + bb1, c1 = f32x2{w[2], w[3]} + bb1;
            const u32x4 pk = {pack_bf16x2(a0.x, a0.y), pack_bf16x2(a1.x, a1.y), pack_bf16x2(c0.x, c0.y),
                              pack_bf16x2(c1.x, c1.y)};
            __builtin_nontemporal_store(pk, reinterpret_cast<u32x4*>(yt + ((mi * 4 + np) * 64 + lane) * 8));
            if constexpr (MODE == 0) {
              ssum[2 * np] += a0 + a1;
              ssq[2 * np] = __builtin_elementwise_fma(a0, a0, __builtin_elementwise_fma(a1, a1, ssq[2 * np]));
              ssum[2 * np + 1] += c0 + c1;
              ssq[2 * np + 1] = __builtin_elementwise_fma(c0, c0, __builtin_elementwise_fma(c1, c1, ssq[2 * np + 1]));
            }
          }
        } else {
#pragma unroll
          for (int mi = 0; mi < 4; ++mi) {
            const bool row_ok = t.y0 + 2 * wave + (mi >> 1) < H;
            const int xb = t.x0 + (mi & 1) * 16 + 4 * g;
            uint32_t hv[8];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              const int nj = 2 * np + h;
              const float bias = h ? b1 : b0;
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const float av = acc[mi][nj][j] + bias;
                hv[4 * h + j] = (uint32_t)f32_to_bf16(av);
                if (MODE == 0 && row_ok && xb + j < W) {
                  ssum[nj].x += av;
                  ssq[nj].x = __builtin_fmaf(av, av, ssq[nj].x);
                }
              }
            }
            *reinterpret_cast<uint4*>(yt + ((mi * 4 + np) * 64 + lane) * 8) =
                make_uint4(hv[0] | (hv[1] << 16), hv[2] | (hv[3] << 16), hv[4] | (hv[5] << 16), hv[6] | (hv[7] << 16));
          }
        }
      }
    } else {
      // BN + ReLU of the bf16-rounded outputs (what the pool kernels read back from y), summed
      // per 16-px fragment row, then per pool bin in a fixed (wave, mi) order
      float* red = (float*)(smem + C4_RED_OFF);  // [wave][mi][128]
      if (tid < 32) {  // bin slot of fragment (wave, mi) = tid: (row bin - first) * 2 + (col bin - first), -1 off image
        const int row = t.y0 + 2 * (tid >> 2) + ((tid & 3) >> 1), col = t.x0 + 16 * (tid & 1);
        sslot[tid] = row < H ? (row / rh - t.y0 / rh) * 2 + (col / rw - t.x0 / rw) : -1;
      }
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int nj = 0; nj < 8; ++nj) {
          const float bias = sbias[16 * nj + r];
          const float2 a = saff[16 * nj + r];
          float s = 0.f;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float vb = bf16_to_f32(f32_to_bf16(acc[mi][nj][j] + bias));
            s += fmaxf(vb * a.x + a.y, 0.f);
          }
          s += __shfl_xor(s, 16);
          s += __shfl_xor(s, 32);
          if (g == 0) red[(wave * 4 + mi) * 128 + 16 * nj + r] = s;
        }
      __syncthreads();
      {
        const int slot = tid >> 7, c = tid & 127;
        float s = 0.f;
        for (int f = 0; f < 32; ++f)
          if (sslot[f] == slot) s += red[f * 128 + c];
        out[(item * 4 + slot) * 128 + c] = s;
      }
      // red / sslot are rewritten only after the next item's 12 step barriers
    }
  }
  if constexpr (MODE == 0) {
    // statistics: lanes of equal r, then the 8 waves in fixed order (the A slots are free: no
    // copy is in flight after the last item)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    float* red = (float*)smem;  // [8 wave][128 n][2]
#pragma unroll
    for (int nj = 0; nj < 8; ++nj) {
      float a = ssum[nj].x + ssum[nj].y, q = ssq[nj].x + ssq[nj].y;
      a += __shfl_xor(a, 16);
      a += __shfl_xor(a, 32);
      q += __shfl_xor(q, 16);
      q += __shfl_xor(q, 32);
      if (g == 0) {
        red[(wave * 128 + 16 * nj + r) * 2] = a;
        red[(wave * 128 + 16 * nj + r) * 2 + 1] = q;
      }
    }
    __syncthreads();
    for (int i = tid; i < C5 * 2; i += 512) {  // channel-major [256][gridDim.x][2] (k_bn_affine cm = 1)
      const int c = i >> 1, k = i & 1;
      float v = 0.f;
      if ((c >> 7) == nh)
        for (int w = 0; w < 8; ++w) v += red[(w * 128 + (c & 127)) * 2 + k];
      out[((long long)c * gridDim.x + blockIdx.x) * 2 + k] = v;
    }
  }
}

// BN + ReLU + AdaptiveAvgPool(4) partial sums over v4's y, 8-row half tiles: when every half tile
// lies inside one pool bin and no bins overlap (H % 32 == 0, W % 128 == 0).  A half tile of one
// channel half is 64 KiB contiguous (waves 4h .. 4h+3 of the item); thread t reads 16-byte chunk
// t + 256k (k = wave x mi), so it keeps channels (np, r) of both h of its lane's chunk -> with
// both channel halves 4 sums; the 4 pixel-quad lanes fold by shuffles at the end.  Split sp of
// bin reg takes the bin's half tiles sp, sp + POOL_SPLIT, ... (raster order).
__global__ __launch_bounds__(256) void k_rp_bn_relu_pool_v4_tiles(const bf16_t* __restrict__ y, int H, int W,
                                                                  const float2* __restrict__ aff,
                                                                  float* __restrict__ part) {
  __shared__ float red[C5];
  const int b = (int)gridDim.y - 1 - (int)blockIdx.y;  // images last-to-first (see conv5 v4's tile order)
  const int reg = blockIdx.x / POOL_SPLIT, sp = blockIdx.x % POOL_SPLIT;
  const int i = reg / 4, j = reg % 4;
  const int tiles_x = W / C4_TW, tiles_y = H / C4_TH;
  const int rhy = H / 32, rtx = W / 128;  // bin size in half tiles (8 rows) and tiles (32 cols)
  const int t = threadIdx.x, lane = t & 63, np = t >> 6, r = lane & 15;
  float2 af[2][2];
#pragma unroll
  for (int nh = 0; nh < 2; ++nh)
#pragma unroll
    for (int h = 0; h < 2; ++h) af[nh][h] = aff[nh * 128 + 32 * np + 16 * h + r];
  float acc[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
  for (int q = sp; q < rhy * rtx; q += POOL_SPLIT) {
    const int hy = i * rhy + q / rtx, tx = j * rtx + q % rtx;  // global half-tile row, tile column
    const long long tile = ((long long)b * tiles_y + (hy >> 1)) * tiles_x + tx;
#pragma unroll
    for (int nh = 0; nh < 2; ++nh) {
      const uint4* src = reinterpret_cast<const uint4*>(y + ((2 * tile + nh) * 8 + 4 * (hy & 1)) * 16 * 512) + t;
      uint4 v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const u32x4 xv = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src + 256 * u));
        v[u] = make_uint4(xv.x, xv.y, xv.z, xv.w);
      }
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const uint32_t w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const float lo = __uint_as_float(w[2 * h + e] << 16), hi = __uint_as_float(w[2 * h + e] & 0xffff0000u);
            acc[nh][h] += fmaxf(lo * af[nh][h].x + af[nh][h].y, 0.f);
            acc[nh][h] += fmaxf(hi * af[nh][h].x + af[nh][h].y, 0.f);
          }
      }
    }
  }
#pragma unroll
  for (int nh = 0; nh < 2; ++nh)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float v = acc[nh][h];
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      if (lane < 16) red[nh * 128 + 32 * np + 16 * h + r] = v;
    }
  __syncthreads();
  part[(((long long)b * 16 + reg) * POOL_SPLIT + sp) * C5 + t] = red[t];
}

// The same over v4's y for any shape (bins may overlap, tiles may be ragged): as
// k_rp_bn_relu_pool_frag with v4's item addressing.
__global__ __launch_bounds__(256) void k_rp_bn_relu_pool_v4_frag(const bf16_t* __restrict__ y, int H, int W,
                                                                 const float2* __restrict__ aff,
                                                                 float* __restrict__ part) {
  __shared__ float red[2][C5];
  const int b = blockIdx.y, reg = blockIdx.x / POOL_SPLIT, sp = blockIdx.x % POOL_SPLIT;
  const int i = reg / 4, j = reg % 4;
  const int cp = threadIdx.x & 127, ql = threadIdx.x >> 7;
  const int nh = cp >> 6, np = (cp >> 4) & 3, r = cp & 15, n0 = nh * 128 + 32 * np + r, n1 = n0 + 16;
  const int ya = (i * H) / 4, yb = ((i + 1) * H + 3) / 4, xa = (j * W) / 4, xb = ((j + 1) * W + 3) / 4;
  const int rows = yb - ya;
  const int r0 = ya + (rows * sp) / POOL_SPLIT, r1 = ya + (rows * (sp + 1)) / POOL_SPLIT;
  const int qa = xa >> 2, nq = ((xb + 3) >> 2) - qa;
  const int tiles_x = (W + C4_TW - 1) / C4_TW, tiles_y = (H + C4_TH - 1) / C4_TH;
  const float2 a0 = aff[n0], a1 = aff[n1];
  float s0 = 0.f, s1 = 0.f;
  constexpr int PU = 8;
  int yy = r0, k = ql;
  while (k >= nq) {
    k -= nq;
    ++yy;
  }
  while (yy < r1) {
    uint4 v[PU];
    int xqs[PU];
    bool ok[PU];
#pragma unroll
    for (int u = 0; u < PU; ++u) {
      ok[u] = yy < r1;
      const int ry = ok[u] ? yy : r1 - 1, xq = (qa + (ok[u] ? k : 0)) * 4;
      xqs[u] = xq;
      const long long tile = ((long long)b * tiles_y + ry / C4_TH) * tiles_x + xq / C4_TW;
      const int ly = ry % C4_TH, lx = xq % C4_TW;
      const int wave = ly >> 1, mi = (ly & 1) * 2 + (lx >> 4), g = (lx & 15) >> 2;
      v[u] = *reinterpret_cast<const uint4*>(y + (((((2 * tile + nh) * 8 + wave) * 4 + mi) * 4 + np) * 64 + g * 16 + r) * 8);
      k += 2;
      while (k >= nq) {
        k -= nq;
        ++yy;
      }
    }
#pragma unroll
    for (int u = 0; u < PU; ++u) {
      const uint32_t w0[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int xx = xqs[u] + e;
        if (ok[u] && xx >= xa && xx < xb) {
          const float c0 = bf16_to_f32((bf16_t)(e & 1 ? w0[e >> 1] >> 16 : w0[e >> 1] & 0xffff));
          const float c1 = bf16_to_f32((bf16_t)(e & 1 ? w0[2 + (e >> 1)] >> 16 : w0[2 + (e >> 1)] & 0xffff));
          s0 += fmaxf(c0 * a0.x + a0.y, 0.f);
          s1 += fmaxf(c1 * a1.x + a1.y, 0.f);
        }
      }
    }
  }
  red[ql][n0] = s0;
  red[ql][n1] = s1;
  __syncthreads();
  const int c = threadIdx.x;
  part[(((long long)b * 16 + reg) * POOL_SPLIT + sp) * C5 + c] = red[0][c] + red[1][c];
}

// MODE 1's pool: pooled[b][c][bin] = the sum of the bin's item partials (tiles in raster order)
// / the bin's pixel count.  grid (16 bins, B), thread = channel.
__global__ __launch_bounds__(256) void k_rp_pool_finish_v4(const float* __restrict__ ip, int B, int H, int W,
                                                           float* __restrict__ pooled) {
  const int b = blockIdx.y, reg = blockIdx.x, i = reg / 4, j = reg % 4, c = threadIdx.x;
  const int nh = c >> 7, cc = c & 127;
  const int rh = H >> 2, rw = W >> 2;
  const int tiles_x = W / C4_TW, tiles_y = (H + C4_TH - 1) / C4_TH;
  const int ty0 = (i * rh) / C4_TH, ty1 = ((i + 1) * rh - 1) / C4_TH;
  const int tx0 = (j * rw) / C4_TW, tx1 = ((j + 1) * rw - 1) / C4_TW;
  float s = 0.f;
  for (int ty = ty0; ty <= ty1; ++ty)
    for (int tx = tx0; tx <= tx1; ++tx) {
      const int slot = (i - (ty * C4_TH) / rh) * 2 + (j - (tx * C4_TW) / rw);
      const long long tile = ((long long)b * tiles_y + ty) * tiles_x + tx;
      s += ip[((2 * tile + nh) * 4 + slot) * 128 + cc];
    }
  pooled[((long long)b * C5 + c) * 16 + reg] = s / (float)(rh * rw);
}

__global__ __launch_bounds__(256) void k_c4_pad_zero(bf16_t* __restrict__ att, int H, int W) {
  c4_pad_body(att, H, W, blockIdx.x, blockIdx.y, gridDim.x);
}

// k_rp_gate: persistent, one 512-thread workgroup per CU over 8x32-pixel tiles
inline int gate_grid(int B, int H, int W) {
  return (int)std::min<long long>((long long)B * ((W + 31) / 32) * ((H + 7) / 8), device_cus());
}

template <int MODE>
int conv5_launch(const bf16_t* att, int B, int H, int W, const char* blob, const Layout& L, const float2* aff5,
                 bf16_t* y, float* out, hipStream_t s) {
  static const hipError_t sattr = hipFuncSetAttribute((const void*)k_rp_conv5_v4<MODE>,
                                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)C4_SMEM);
  if (sattr != hipSuccess) return (int)sattr;
  const int gcv = conv4_grid(B, H, W);
  k_rp_conv5_v4<MODE><<<gcv, 512, C4_SMEM, s>>>(att, B, H, W, blob, L, aff5, y, out, gcv % 16 == 0);
  return RGBD_OK;
}

}  // namespace

namespace rgbd::rp {

int gate(const bf16_t* fus, int B, int H, int W, const char* blob, const Layout& L, const float2* aff2, bf16_t* att,
         hipStream_t s) {
  TimerScope ts("rp_chain", s);
  static const hipError_t gattr =
      hipFuncSetAttribute((const void*)k_rp_gate, hipFuncAttributeMaxDynamicSharedMemorySize, (int)GT_SMEM);
  if (gattr != hipSuccess) return (int)gattr;
  k_rp_gate<<<gate_grid(B, H, W), 512, GT_SMEM, s>>>(fus, B, H, W, blob, L, aff2, att);
  return RGBD_OK;
}

int c4_pad_zero(bf16_t* att, int B, int H, int W, hipStream_t s) {
  k_c4_pad_zero<<<dim3(8, B * 4), 256, 0, s>>>(att, H, W);
  return RGBD_OK;
}

long long conv4_tiles(int B, int H, int W) {
  return (long long)B * ((W + C4_TW - 1) / C4_TW) * ((H + C4_TH - 1) / C4_TH);
}
// persistent, one 147 KB-LDS workgroup per CU, in pairs (the two channel halves of a tile)
int conv4_grid(int B, int H, int W) { return 2 * (int)std::min<long long>(conv4_tiles(B, H, W), device_cus() / 2); }
// eval: BN + ReLU + AdaptiveAvgPool(4) in conv5's epilogue when the pool bins do not overlap and
// every 16-px fragment row of a 16x32 tile lies in one bin, a tile in at most 2 x 2 bins
bool conv4_pool_fused(int H, int W) { return H % 4 == 0 && W % 64 == 0 && H >= 64 && W >= 128; }

// MODE 0: y + BN statistics -> out (slab); 1: per-item bin partials -> out, no y; 2: y only
int conv5_v4(int mode, const bf16_t* att, int B, int H, int W, const char* blob, const Layout& L, const float2* aff5,
             bf16_t* y, float* out, hipStream_t s) {
  TimerScope ts("rp_conv3x3", s);
  return mode == 0   ? conv5_launch<0>(att, B, H, W, blob, L, aff5, y, out, s)
         : mode == 1 ? conv5_launch<1>(att, B, H, W, blob, L, aff5, y, out, s)
                     : conv5_launch<2>(att, B, H, W, blob, L, aff5, y, out, s);
}

// BN + ReLU + AdaptiveAvgPool(4) partial sums over conv5 v4's y (MODE 0 / 2)
int pool_v4(const bf16_t* y, int B, int H, int W, const float2* aff5, float* part, hipStream_t s) {
  if (H % 32 == 0 && W % 128 == 0)
    k_rp_bn_relu_pool_v4_tiles<<<dim3(16 * POOL_SPLIT, B), 256, 0, s>>>(y, H, W, aff5, part);
  else
    k_rp_bn_relu_pool_v4_frag<<<dim3(16 * POOL_SPLIT, B), 256, 0, s>>>(y, H, W, aff5, part);
  return RGBD_OK;
}

int pool_finish_v4(const float* ip, int B, int H, int W, float* pooled, hipStream_t s) {
  k_rp_pool_finish_v4<<<dim3(16, B), 256, 0, s>>>(ip, B, H, W, pooled);
  return RGBD_OK;
}

}  // namespace rgbd::rp

#ifdef RGBD_DIAG
extern "C" int rgbd_debug_conv5_stamps(void* buf) {
  unsigned long long* p = (unsigned long long*)buf;
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_c4_stamps), &p, sizeof(p));
}
#endif
