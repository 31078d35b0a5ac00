// K5, bf16 dW: the code-merged weight gradient as a persistent LDS-DMA MFMA GEMM over a
// device-built plan, a fold of its per-item partials into the five filters, and the bias channel
// sums.  The host plan / workspace arithmetic and the launch functions (dsam_common.hpp) follow
// the kernels.
#include "dsam_common.hpp"

using namespace rgbd;
using namespace rgbd::k5;

namespace {

// bf16 dW, code-merged:
//   dW_k[o][tap][c] = sum over output px p with code(src(p, tap)) == k of G[p][o] X[src][c]
// for every region code k present, folded by k_dsam_wgrad_fold into the five filters (conv_i
// gets the codes with bit i, proj gets all): work ~ one dense dW instead of popcount + 1 of them.
// A unit is 64 raster-consecutive output pixels of one image.  Load balance: one code (the
// remainder region) typically meets every unit while the others meet a few percent, so
// wg_plan_body builds per-code lists of live units (code_presence_body) and cuts them into items of
// about equal length; wg_masks_body precomputes, per list entry and tap, the 64-bit mask of the
// unit's pixels whose source meets code k; k_dsam_wgrad_mm runs persistently over
// (item, output tile) work.
//
// Output tile: 32*FM channels (o) x 128 kk (kk = tap*Cin + c: four 32-wide blocks, each inside
// one tap), 4 waves as 2x2 (wave tile 16*FM x 64); one unit (64 px = two MFMA k-blocks) per
// step, operands by LDS-DMA in an S-deep ring, S-1 steps ahead:
//   G  [64 px][32*FM o] from the NHWC upstream gradient (FM blocks of 64-byte rows),
//   X  [64 px][4 x 32 c] im2col rows from the NHWC input; every row copies a valid (clamped)
//      pixel and the rows outside the input, past the image or of another code are zeroed in
//      registers from the entry's tap masks (staged in LDS with the item's unit ids).
// Both MFMA operands are read with ds_read_b64_tr_b16 ([px][col] -> k-major fragments); rows are
// XOR-swizzled by row bit 3 so the 32-lane halves of a transposed read fall on disjoint banks.
constexpr int WPX = 64;        // output pixels per unit / step
constexpr int WITEM_MAX = 64;  // units per item (LDS staging of ids + masks)
typedef __attribute__((ext_vector_type(4))) short v4s;

template <int FM>
struct WgCfg {
  static constexpr int S = FM == 6 ? 3 : 4;
  static constexpr int NBLK = FM + 4;            // 4 KB blocks per stage: FM of G, 4 of X
  static constexpr int STAGE = NBLK * WPX * 64;
  static constexpr int PER = NBLK;               // DMA pieces per wave per step
  static constexpr int OFF_UNITS = S * STAGE;    // [WITEM_MAX] int unit ids
  static constexpr int OFF_MASKS = OFF_UNITS + WITEM_MAX * 4;  // [WITEM_MAX][9] u64 tap masks
  static constexpr size_t SMEM = (size_t)OFF_MASKS + WITEM_MAX * 9 * 8;
  static_assert(SMEM <= 163840, "dW LDS budget");
};

__device__ __forceinline__ int wg_swz(int row) { return ((row >> 3) & 1) << 1; }

struct WgArgs {
  const bf16_t* gout;     // NHWC [B][ho][wo][Cout]
  const bf16_t* x;        // NHWC [B][h][w][Cin]
  const uint8_t* code;    // [B][h][w]
  const uint16_t* pres;   // [B * nunit] bit k: code k met by the unit's sources
  int* list;              // [<= 16 * B * nunit] live entries: unit | code << 24, by code then unit
  unsigned long long* masks;  // [entry][9] tap masks of the entry's unit for its code
  int4* items;            // [<= 16 * B * nunit] (code, first entry, end entry, -)
  int* counts;            // [0] live entries, [1] items
  int B, Cin, h, w, Cout, ho, wo, nunit, ntile_kk, ntile_o, target;
  float inv_wo;
  const bf16_t* zero;     // LD_ZERO_BYTES of zeros (rows the im2col gather masks out)
  float* partial;         // [item][Cout][9*Cin] f32
};

__device__ __forceinline__ void code_presence_body(const uint8_t* __restrict__ code, int B, int h, int w,
                                                   uint16_t* __restrict__ pres, int block) {
  // one wave per 64-px unit: OR of 1 << code over its 9-tap sources
  const int ho = (h + 1) / 2, wo = (w + 1) / 2, hwo = ho * wo, nunit = (hwo + WPX - 1) / WPX;
  const long long u = (block * (long long)blockDim.x + threadIdx.x) >> 6;
  const int l = threadIdx.x & 63;
  uint32_t m = 0u;
  if (u < (long long)B * nunit) {
    const int b = (int)(u / nunit), p = (int)(u % nunit) * WPX + l;
    if (p < hwo) {
      const int oy = p / wo, ox = p % wo;
      uint32_t cv[9];
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int iy = 2 * oy - 1 + tap / 3, ix = 2 * ox - 1 + tap % 3;
        const bool ok = iy >= 0 && iy < h && ix >= 0 && ix < w;
        cv[tap] = code[((long long)b * h + (ok ? iy : 0)) * w + (ok ? ix : 0)];  // unconditional: one round trip
        cv[tap] = ok ? 1u << cv[tap] : 0u;
      }
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) m |= cv[tap];
    }
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) m |= (uint32_t)__shfl_xor((int)m, o);
  if (l == 0 && u < (long long)B * nunit) {
    pres[u] = (uint16_t)m;
  }
}

// Plan (one 1024-thread workgroup): per code the ordered list of live units, then items of
// about equal length L = ceil(entries / (target / output tiles)), capped at WITEM_MAX.
constexpr int WG_PRES_LDS = 8192;  // presence entries k_wg_plan keeps in LDS
__device__ __forceinline__ void wg_plan_body(const WgArgs& a) {
  __shared__ int cnt_s[16], off_s[17];
  if (threadIdx.x < LD_ZERO_BYTES / 16)
    reinterpret_cast<uint4*>(const_cast<bf16_t*>(a.zero))[threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
  __shared__ uint16_t spres[WG_PRES_LDS];  // the compaction pass re-reads presence from LDS
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int U = a.B * a.nunit;
  const bool in_lds = U <= WG_PRES_LDS;
  if (tid < 16) cnt_s[tid] = 0;
  __syncthreads();
  // counts per code
  uint32_t c16[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) c16[k] = 0u;
  for (int u = tid; u < U; u += 1024) {
    const uint32_t m = a.pres[u];
    if (in_lds) spres[u] = (uint16_t)m;
#pragma unroll
    for (int k = 0; k < 16; ++k) c16[k] += (m >> k) & 1u;
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    uint32_t v = c16[k];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += (uint32_t)__shfl_xor((int)v, o);
    if (lane == 0 && v) atomicAdd(&cnt_s[k], (int)v);
  }
  __syncthreads();
  if (tid == 0) {
    int o = 0;
    for (int k = 0; k < 16; ++k) {
      off_s[k] = o;
      o += cnt_s[k];
    }
    off_s[16] = o;
  }
  __syncthreads();
  // ordered compaction, all 16 codes per pass: wave ballots -> per-(code, wave) counts ->
  // exclusive offsets; units keep their order within each code
  __shared__ int wc[16][16], wpre[16][16], cbase[16], ctot[16];
  if (tid < 16) cbase[tid] = off_s[tid];
  for (int u0 = 0; u0 < U; u0 += 1024) {
    const int u = u0 + tid;
    const uint32_t m = u < U ? (in_lds ? (uint32_t)spres[u] : (uint32_t)a.pres[u]) : 0u;
    unsigned long long bal[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      bal[k] = __ballot((m >> k) & 1u);
      if (lane == 0) wc[k][w] = __popcll(bal[k]);
    }
    __syncthreads();
    if (tid < 256) {
      const int k = tid >> 4, q = tid & 15;
      int pre = 0;
      for (int i = 0; i < q; ++i) pre += wc[k][i];
      wpre[k][q] = pre;
      if (q == 15) ctot[k] = pre + wc[k][15];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if ((m >> k) & 1u)
        a.list[cbase[k] + wpre[k][w] + __popcll(bal[k] & ((1ull << lane) - 1ull))] = u | (k << 24);
    __syncthreads();
    if (tid < 16) cbase[tid] += ctot[tid];
    __syncthreads();
  }
  // items: code k's c live units cut into n_k = ceil(c / L) near-equal runs, emitted in parallel
  __shared__ int ibase[17];
  const int total = off_s[16];
  const int want = max(1, a.target / max(1, a.ntile_kk * a.ntile_o));
  const int L = min(max(1, (total + want - 1) / want), WITEM_MAX);
  if (tid == 0) {
    int ni = 0;
    for (int k = 0; k < 16; ++k) {
      ibase[k] = ni;
      ni += (cnt_s[k] + L - 1) / L;
    }
    ibase[16] = ni;
    a.counts[0] = total;
    a.counts[1] = ni;
    a.counts[2] = 0;  // k_dsam_wgrad_mm's next-work counter
    a.counts[3] = 0;  // ... and its next channel-sum unit (fold)
  }
  __syncthreads();
  for (int it = tid; it < ibase[16]; it += 1024) {
    int k = 0;
    while (it >= ibase[k + 1]) ++k;
    const int c = cnt_s[k], n = ibase[k + 1] - ibase[k], j = it - ibase[k];
    a.items[it] = make_int4(k, off_s[k] + (int)((long long)c * j / n), off_s[k] + (int)((long long)c * (j + 1) / n), 0);
  }
}

// Tap masks of every live entry: one wave per entry, lane = pixel of the unit.
__device__ __forceinline__ void wg_masks_body(const WgArgs& a, int block) {
  const int e = (block * 256 + threadIdx.x) >> 6, l = threadIdx.x & 63;
  if (e >= a.counts[0]) return;  // wave-uniform
  const int v = a.list[e], u = v & 0xffffff, k = v >> 24;
  const int hwo = a.ho * a.wo, b = u / a.nunit, p = (u % a.nunit) * WPX + l;
  const bool pv = p < hwo;
  const int oy = pv ? p / a.wo : 0, ox = pv ? p % a.wo : 0;
  uint32_t cv[9];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int iy = 2 * oy - 1 + tap / 3, ix = 2 * ox - 1 + tap % 3;
    const bool ok = pv && iy >= 0 && iy < a.h && ix >= 0 && ix < a.w;
    cv[tap] = a.code[((long long)b * a.h + (ok ? iy : 0)) * a.w + (ok ? ix : 0)];  // unconditional: one round trip
    cv[tap] = ok ? cv[tap] : 0xffu;
  }
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const unsigned long long m = __ballot(cv[tap] == (uint32_t)k);
    if (l == 0) a.masks[(long long)e * 9 + tap] = m;
  }
}

// The dW planning of up to WG_MAXLEG legs in three launches (blockIdx.z = leg; blocks past a
// leg's own count exit): unit presence, the per-code lists and items, the tap masks.
struct WgLegs {
  WgArgs a[WG_MAXLEG];
  int max_entries[WG_MAXLEG];
  int n;
};
__global__ __launch_bounds__(256) void k_code_presence_legs(const WgLegs L) {
  const WgArgs& a = L.a[blockIdx.z];
  if ((long long)blockIdx.x * 256 >= (long long)a.B * a.nunit * 64) return;  // block-uniform
  code_presence_body(a.code, a.B, a.h, a.w, const_cast<uint16_t*>(a.pres), blockIdx.x);
}
__global__ __launch_bounds__(1024) void k_wg_plan_legs(const WgLegs L) { wg_plan_body(L.a[blockIdx.z]); }
__global__ __launch_bounds__(256) void k_wg_masks_legs(const WgLegs L) {
  const WgArgs& a = L.a[blockIdx.z];
  if ((long long)blockIdx.x * 4 >= L.max_entries[blockIdx.z]) return;  // block-uniform
  wg_masks_body(a, blockIdx.x);
}

// out[(split*B + b)*C + c] = sum over pixel range `split` of g[b][p][c], NHWC bf16 g: workgroup
// (b, 64 channels, split), thread = channel pair x one of 8 pixel strides, fixed-order combine.
__host__ __device__ inline int chan_sum_splits(int HW) {
  const int sp = HW / 256;
  return sp < 1 ? 1 : (sp > CS_SPLIT_MAX ? CS_SPLIT_MAX : sp);
}
// one workgroup's share: image b, channels [64 cb, 64 cb + 64), pixel range sp of nsp
__device__ __forceinline__ void chan_sum_body(const bf16_t* __restrict__ g, int HW, int C, int B, int b, int cb,
                                              int sp, int nsp, float* __restrict__ out, float2 (*red)[32]) {
  const int cp = threadIdx.x & 31, sub = threadIdx.x >> 5;
  const int c = cb * 64 + 2 * cp;
  const int p0 = (int)((long long)sp * HW / nsp), p1 = (int)((long long)(sp + 1) * HW / nsp);
  float2 acc = make_float2(0.f, 0.f);
  if (c < C) {
    const bf16_t* base = g + (long long)b * HW * C + c;
#pragma unroll 4
    for (int p = p0 + sub; p < p1; p += 8) {
      const uint32_t u = *reinterpret_cast<const uint32_t*>(base + (long long)p * C);
      acc.x += __uint_as_float(u << 16);
      acc.y += __uint_as_float(u & 0xffff0000u);
    }
  }
  red[sub][cp] = acc;
  __syncthreads();
  if (sub == 0 && c < C) {
    float2 t = red[0][cp];
    for (int q = 1; q < 8; ++q) {
      t.x += red[q][cp].x;
      t.y += red[q][cp].y;
    }
    float* o = out + ((long long)sp * B + b) * C + c;
    o[0] = t.x;
    if (c + 1 < C) o[1] = t.y;
  }
}
// NL legs of one output tile shape in one persistent launch: every workgroup drains leg 0's work
// counter, then leg 1's, ..., so legs that are ready together share the CUs instead of queueing
// whole-chip launches behind each other (the loop body is instantiated per leg: each leg's
// arguments stay scalar kernel arguments).
//
// With fold set, the workgroups then drain the legs' bias channel sums (chan_sum_body units of the
// upstream gradient, counter counts[3]) — work that would otherwise be one more launch after the
// GEMM's drain tail.
template <int NL>
struct WgMulti {
  WgArgs a[NL];
  float* csum[NL];  // [nsplit][B][Cout] channel sums (fold)
  int n;            // legs in use, 1..NL
  int fold;
};

template <int FM, int NL>
__global__ __launch_bounds__(256) void k_dsam_wgrad_mm(const WgMulti<NL> L) {
  using Cfg = WgCfg<FM>;
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  int* sunits = (int*)(smem + Cfg::OFF_UNITS);
  unsigned long long* smasks = (unsigned long long*)(smem + Cfg::OFF_MASKS);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int wm = wave & 1, wn = wave >> 1;
  const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
  // per-lane copy roles: pixel row pr of every block, 16-byte chunk q
  const int pr = 16 * wave + (lane >> 2);
  const int qch = 8 * ((lane & 3) ^ wg_swz(pr));
  // transposed fragment [k = 8g + j][col = c0 + r] of a [64 px][32 col] block (64-byte rows): the
  // XOR swizzle term depends on row bit 3 = g & 1 only, so every read of a lane is its base
  // address plus a compile-time offset
  const int q4 = (lane & 15) >> 2, p4 = lane & 3;
  const int trow = 8 * g + q4;
  const int tbase0 = trow * 64 + 16 * ((p4 >> 1) ^ wg_swz(trow)) + (4 * p4 & 7) * 2;        // c0 = 0
  const int tbase16 = trow * 64 + 16 * ((2 | (p4 >> 1)) ^ wg_swz(trow)) + (4 * p4 & 7) * 2;  // c0 = 16
  typedef __attribute__((address_space(3))) char lds_char;
  typedef __attribute__((address_space(3))) v4s lds_v4s;
  lds_char* const lsm = (lds_char*)smem;  // one generic -> LDS conversion, not one per read
  lds_char* b0 = lsm;   // this step's slot + the lane's base, per c0
  lds_char* b16 = lsm;
  auto trfrag = [&](int blk, int kb, int c0) {  // blk: block byte offset in the slot; c0 in {0, 16}
    lds_char* p = (c0 ? b16 : b0) + blk + kb * 32 * 64;
    const v4s t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)p);
    const v4s t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(p + 4 * 64));
    Frag<bf16_t> f;
    const uint2 u0 = __builtin_bit_cast(uint2, t0), u1 = __builtin_bit_cast(uint2, t1);
    f.v = make_uint4(u0.x, u0.y, u1.x, u1.y);
    return f;
  };
  int* next_s = (int*)(smem + Cfg::OFF_UNITS) + WITEM_MAX - 1;  // unit ids are staged after the read
  auto run_leg = [&](const WgArgs& a) {
    const int KK = 9 * a.Cin, hwo = a.ho * a.wo, ntile = a.ntile_kk * a.ntile_o;
    const int nwork = a.counts[1] * ntile;
    for (;;) {
      // dynamic assignment of (item, tile) work: items differ in live units per code
      __syncthreads();
      if (tid == 0) *next_s = __hip_atomic_fetch_add(a.counts + 2, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __syncthreads();
      const int wi = *next_s;
      __syncthreads();  // every thread has it before the unit ids overwrite the slot
      if (wi >= nwork) break;
      const int4 item = a.items[wi / ntile];
      const int tile = wi % ntile, e0 = item.y, nst = item.z - item.y;
      const int kk0 = (tile % a.ntile_kk) * 128, o0 = (tile / a.ntile_kk) * 32 * FM;
      // stage the item's unit ids and tap masks
      for (int i = tid; i < nst; i += 256) sunits[i] = a.list[e0 + i] & 0xffffff;
      for (int i = tid; i < nst * 9; i += 256) smasks[i] = a.masks[(long long)e0 * 9 + i];
      __syncthreads();
      // X block j: (tap, channel offset) uniform; source offset dy*w + dx from the row's origin
      int xtap[4], xoff[4], xc[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int kk = kk0 + 32 * j;
        const bool ok = kk < KK;
        xtap[j] = ok ? kk / a.Cin : -1;
        const int tp = ok ? xtap[j] : 0;
        xoff[j] = (tp / 3) * a.w + tp % 3;
        xc[j] = ok ? kk % a.Cin : 0;
      }
      const bf16_t* zrow = a.zero + qch;
      // One step = one unit: G rows (its 64 output pixels) and X rows (their im2col sources).  A
      // row of X whose source is outside the input, past the image, or of another code than the
      // item's reads the zero row: it contributes exactly zero, no masking in registers.
      auto issue = [&](int slot, int it) {
        const int u = __builtin_amdgcn_readfirstlane(sunits[it]);
        const int b = u / a.nunit;
        const int p = (u - b * a.nunit) * WPX + pr;
        const int pc = p < hwo ? p : hwo - 1;
        const int oy = (int)(((float)pc + 0.5f) * a.inv_wo), ox = pc - oy * a.wo;
        const uint32_t sb = lds0 + slot * Cfg::STAGE + wave * 1024;
        const bf16_t* gsrc = a.gout + ((long long)b * hwo + pc) * a.Cout + qch;
#pragma unroll
        for (int ob = 0; ob < FM; ++ob) dma_lds16(gsrc + min(o0 + 32 * ob, a.Cout - 32), sb + ob * 4096);
        const int org = (b * a.h + 2 * oy - 1) * a.w + 2 * ox - 1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const unsigned long long m = xtap[j] >= 0 ? smasks[it * 9 + xtap[j]] : 0ull;
          const bool live = (m >> pr) & 1ull;
          const bf16_t* src = live ? a.x + (long long)(org + xoff[j]) * a.Cin + xc[j] + qch : zrow;
          dma_lds16(src, sb + (FM + j) * 4096);
        }
      };
      f32x4 acc[FM][4];
#pragma unroll
      for (int mi = 0; mi < FM; ++mi)
#pragma unroll
        for (int nj = 0; nj < 4; ++nj) acc[mi][nj] = f32x4{0.f, 0.f, 0.f, 0.f};
      const int npro = nst < Cfg::S - 1 ? nst : Cfg::S - 1;
      for (int i = 0; i < npro; ++i) issue(i, i);
      if (npro >= 3) vm_wait_barrier<2 * Cfg::PER>();
      else if (npro == 2) vm_wait_barrier<Cfg::PER>();
      else vm_wait_barrier<0>();
#pragma unroll 1
      for (int s = 0; s < nst; ++s) {
        if (s + Cfg::S - 1 < nst) issue((s + Cfg::S - 1) % Cfg::S, s + Cfg::S - 1);
        int st = (s % Cfg::S) * Cfg::STAGE;
        asm volatile("" : "+s"(st));  // no strength reduction of the slot offset into per-read registers
        b0 = lsm + st + tbase0;
        b16 = lsm + st + tbase16;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
          Frag<bf16_t> fa[FM], fb[4];
#pragma unroll
          for (int mi = 0; mi < FM; ++mi) {
            const int ol = wm * 16 * FM + 16 * mi;
            fa[mi] = trfrag((ol >> 5) * 4096, kb, ol & 31);
          }
#pragma unroll
          for (int nj = 0; nj < 4; ++nj) {
            const int kl = wn * 64 + 16 * nj;
            fb[nj] = trfrag((FM + (kl >> 5)) * 4096, kb, kl & 31);
          }
#pragma unroll
          for (int mi = 0; mi < FM; ++mi)
#pragma unroll
            for (int nj = 0; nj < 4; ++nj) mma(acc[mi][nj], fa[mi], fb[nj]);
        }
        const int ahead = (nst - 1 < s + Cfg::S - 1 ? nst - 1 : s + Cfg::S - 1) - (s + 1);
        if (ahead >= 2) vm_wait_barrier<2 * Cfg::PER>();
        else if (ahead == 1) vm_wait_barrier<Cfg::PER>();
        else vm_wait_barrier<0>();
      }
      float* dst = a.partial + ((long long)(wi / ntile) * a.Cout) * KK;
#pragma unroll
      for (int mi = 0; mi < FM; ++mi)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int o = o0 + wm * 16 * FM + 16 * mi + 4 * g + reg;
#pragma unroll
          for (int nj = 0; nj < 4; ++nj) {
            const int c = kk0 + wn * 64 + 16 * nj + r;
            if (o < a.Cout && c < KK) dst[(long long)o * KK + c] = acc[mi][nj][reg];
          }
        }
      __syncthreads();  // staged ids / masks and the ring are free for the next work unit
    }
  };
#pragma unroll
  for (int l = 0; l < NL; ++l)
    if (l < L.n) run_leg(L.a[l]);
  if (!L.fold) return;
  float2(*red)[32] = reinterpret_cast<float2(*)[32]>(smem);  // the ring is free: every wave left the loop
#pragma unroll
  for (int l = 0; l < NL; ++l) {
    if (l >= L.n) break;
    const WgArgs& a = L.a[l];
    const int hwo = a.ho * a.wo, nsp = chan_sum_splits(hwo), ncb = (a.Cout + 63) / 64;
    const int nunit = a.B * ncb * nsp;
    for (;;) {
      __syncthreads();
      if (tid == 0) *next_s = __hip_atomic_fetch_add(a.counts + 3, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __syncthreads();
      const int u = *next_s;
      if (u >= nunit) break;  // uniform: every thread read the same slot
      const int b = u % a.B, cb = (u / a.B) % ncb, sp = u / (a.B * ncb);
      chan_sum_body(a.gout, hwo, a.Cout, a.B, b, cb, sp, nsp, L.csum[l], red);
    }
  }
}

// dW_k (per item partials) -> the reference filters, fixed summation order (items in list
// order: codes ascending, units ascending).
struct CombArgs {
  const float* partial;
  const int4* items;
  const int* counts;
  int Cin, Cout;
  float* dconv_w;
  float* dproj_w;
  const float* csum;
  const rgbd_decomp_info* info;
  int B, nsplit;
  float* dbias;
};
// One block per (output channel o, 32-channel chunk of the input): 72 threads each own four
// consecutive kk of one tap and walk the items in list order (the summation order of the former
// one-block-per-row combine, so the same bits), the chunk's five [9 tap][32 c] rows are parked in LDS (5.6 KB) and written back as five
// contiguous (c, tap) runs of 288 floats.  A block is small, so many are resident per CU and the
// partial reads stream at HBM speed (the per-row form needs 5 x 9 Cin floats of LDS per block:
// two blocks per CU).  Blocks of chunk 0 also write o's bias gradients.  grid (Cin / 32, Cout, legs).
constexpr int FOLD_C = 32, FOLD_T = 128;
__device__ __forceinline__ void fold_body(const CombArgs& A, int o, int c0, float (*srow)[9 * FOLD_C]) {
  const float* __restrict__ partial = A.partial;
  const int4* __restrict__ items = A.items;
  const int Cin = A.Cin, Cout = A.Cout, KK = 9 * Cin, ni = A.counts[1];
  const int t = threadIdx.x;
  if (t < 9 * FOLD_C / 4) {
    const int tap = t / (FOLD_C / 4), q = t % (FOLD_C / 4);
    const long long kk = (long long)tap * Cin + c0 + 4 * q;
    const float* src = partial + (long long)o * KK + kk;
    const long long istr = (long long)Cout * KK;
    float4 seg[4], pr = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < 4; ++i) seg[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    auto acc = [&](const float4 v, int k) {
      pr.x += v.x; pr.y += v.y; pr.z += v.z; pr.w += v.w;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if ((k >> i) & 1) {
          seg[i].x += v.x; seg[i].y += v.y; seg[i].z += v.z; seg[i].w += v.w;
        }
    };
    int it = 0;
    for (; it + 8 <= ni; it += 8) {
      float4 v[8];
      int k[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        v[j] = *reinterpret_cast<const float4*>(src + (it + j) * istr);
        k[j] = items[it + j].x;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) acc(v[j], k[j]);
    }
    for (; it < ni; ++it) acc(*reinterpret_cast<const float4*>(src + it * istr), items[it].x);
    const int r = tap * FOLD_C + 4 * q;
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<float4*>(&srow[i][r]) = seg[i];
    *reinterpret_cast<float4*>(&srow[4][r]) = pr;
  }
  __syncthreads();
  // OIHW: element (o, c0 + c, tap) at o * KK + (c0 + c) * 9 + tap — a contiguous run per filter
  for (int e = t; e < 5 * 9 * FOLD_C; e += FOLD_T) {
    const int i = e / (9 * FOLD_C), f = e % (9 * FOLD_C), c = f / 9, tap = f % 9;
    const float v = srow[i][tap * FOLD_C + c];
    if (i < 4)
      A.dconv_w[((long long)i * Cout + o) * KK + (long long)c0 * 9 + f] = v;
    else
      A.dproj_w[(long long)o * KK + (long long)c0 * 9 + f] = v;
  }
  // o's bias gradients (csum [nsplit][B][Cout]; conv_layers[i] only where i < len(masks)): the
  // former combine's wave sums, waves 0 / 1 taking i = 0, 2 / 1, 3
  if (c0 == 0 && A.dbias) {
    const int wv = t >> 6, lane = t & 63;
    for (int i = wv; i < 4; i += FOLD_T / 64) {
      float sb = 0.f;
      for (int q = lane; q < A.nsplit * A.B; q += 64) {
        const int b = q % A.B;
        if (i < A.info[b].n_masks) sb += A.csum[(long long)q * Cout + o];
      }
      sb = wave_sum(sb);
      if (lane == 0) A.dbias[i * Cout + o] = sb;
    }
  }
}
__global__ __launch_bounds__(FOLD_T) void k_dsam_wgrad_fold(const CombArgs A0, const CombArgs A1) {
  __shared__ __attribute__((aligned(16))) float srow[5][9 * FOLD_C];
  const CombArgs& A = blockIdx.z == 0 ? A0 : A1;
  if ((int)blockIdx.y >= A.Cout || (int)blockIdx.x * FOLD_C >= A.Cin) return;  // block-uniform
  fold_body(A, blockIdx.y, blockIdx.x * FOLD_C, srow);
}

// ------------------------------------------------------------------ host: plan and launches
// ---- bf16 dW: output tile (FM); items and their partials are sized by the device plan, the
// workspace by the worst case (every code live in every unit)
struct WgPlan {
  int fm, nunit, ntile_kk, ntile_o, max_entries;
};
int wg_fm(int Cout) { return Cout % 192 == 0 ? 6 : (Cout % 128 == 0 ? 4 : 2); }
static WgPlan wg_plan(int B, int Cin, int h, int w, int Cout) {
  WgPlan p;
  p.fm = wg_fm(Cout);
  const int hwo = ((h + 1) / 2) * ((w + 1) / 2);
  p.nunit = (hwo + WPX - 1) / WPX;
  p.ntile_kk = ceil_div(9ll * Cin, 128);
  p.ntile_o = ceil_div(Cout, 32 * p.fm);
  p.max_entries = 16 * B * p.nunit;
  return p;
}
// items are at most max_entries; the plan targets about one work unit per CU (every unit writes an
// f32 partial tile the combine re-reads, so more units cost more than the balance they buy): 256,
// 384 for layers with many output tiles (dsam2's 108: units of ~3 items balance better under the
// dynamic assignment), 192 for layers with few (dsam0's 7) — measured per layer at 640x480
static int wg_target(const WgPlan& p) {
  const int tiles = p.ntile_kk * p.ntile_o;
  return tiles >= 64 ? 384 : (tiles <= 8 ? 192 : 256);
}
// partial buffer bound: items <= entries / L + 16 with L >= entries / (target / tiles)
static size_t wg_max_items(const WgPlan& p) {
  const long long want = std::max(1, wg_target(p) / std::max(1, p.ntile_kk * p.ntile_o));
  return (size_t)std::min<long long>(p.max_entries, want + 16 + p.max_entries / WITEM_MAX);
}

template <int FM, int NL>
hipError_t launch_wg(const WgMulti<NL>& m, int grid, hipStream_t s) {
  static const hipError_t attr = hipFuncSetAttribute((const void*)k_dsam_wgrad_mm<FM, NL>,
                                                     hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     (int)WgCfg<FM>::SMEM);
  if (attr != hipSuccess) return attr;
  k_dsam_wgrad_mm<FM, NL><<<grid, 256, WgCfg<FM>::SMEM, s>>>(m);
  return hipSuccess;
}
template <int NL>
hipError_t launch_wg_fm(int fm, const WgMulti<NL>& m, hipStream_t s) {
  const int grid = 256;  // persistent: one LDS-bound workgroup per CU
  return fm == 6 ? launch_wg<6, NL>(m, grid, s) : fm == 4 ? launch_wg<4, NL>(m, grid, s) : launch_wg<2, NL>(m, grid, s);
}
// bf16 dW plan (rgbd_dsam_plan_size(RGBD_LEG_DW) = total): [presence table [B][units] u16 | 256
// spare bytes | live entry list | their tap masks | items | counters | zero row]
struct WgPlanWs {
  size_t pres, list, masks, items, counts, zero, total;
};
static WgPlanWs wg_plan_ws(const WgPlan& p, int B) {
  WgPlanWs o;
  size_t off = 0;
  o.pres = off;
  off += align256(sizeof(uint16_t) * (size_t)B * p.nunit) + 256;
  o.list = off;
  off += align256(sizeof(int) * (size_t)p.max_entries);
  o.masks = off;
  off += align256(sizeof(unsigned long long) * 9 * p.max_entries);
  o.items = off;
  off += align256(sizeof(int4) * wg_max_items(p));
  o.counts = off;
  off += 256;
  o.zero = off;
  off += LD_ZERO_BYTES;
  o.total = off;
  return o;
}
// dW launch arguments of a bf16 leg over its plan and its run workspace (the partials): both NULL
// with the data pointers when only planning (rgbd_dsam_plan)
static WgArgs wg_args(const WgPlan& P, char* plan, void* ws, const void* gout_nhwc, const void* x_nhwc,
                      const uint8_t* code, int B, int Cin, int h, int w, int Cout) {
  const WgPlanWs L = wg_plan_ws(P, B);
  WgArgs a;
  a.gout = (const bf16_t*)gout_nhwc;
  a.x = (const bf16_t*)x_nhwc;
  a.code = code;
  a.pres = (uint16_t*)(plan + L.pres);
  a.list = (int*)(plan + L.list);
  a.masks = (unsigned long long*)(plan + L.masks);
  a.items = (int4*)(plan + L.items);
  a.counts = (int*)(plan + L.counts);
  a.B = B; a.Cin = Cin; a.h = h; a.w = w; a.Cout = Cout;
  a.ho = (h + 1) / 2; a.wo = (w + 1) / 2;
  a.nunit = P.nunit;
  a.ntile_kk = P.ntile_kk;
  a.ntile_o = P.ntile_o;
  a.target = wg_target(P);
  a.inv_wo = 1.0f / (float)a.wo;
  a.zero = (const bf16_t*)(plan + L.zero);
  a.partial = (float*)ws;
  return a;
}
static bool wg_shape_ok(int B, int Cin, int h, int w, int Cout, const WgPlan& P) {
  const long long hwo = (long long)((h + 1) / 2) * ((w + 1) / 2);
  return Cin % 32 == 0 && Cout % 32 == 0 && hwo < (1ll << 22) && (long long)B * h * w < (1ll << 31) &&
         (long long)B * P.nunit < (1 << 24);
}
static_assert(FOLD_C == 32, "Cin % 32 == 0 is also what the fold's FOLD_C-channel chunks need");
// the code-dependent part of n dW legs: unit presence, the per-code live lists and items, tap
// masks — three launches for all legs
static void wg_plan_launch(int n, const WgArgs* a, const WgPlan* P, hipStream_t s) {
  WgLegs L = {};
  L.n = n;
  long long pres_blocks = 1, mask_blocks = 1;
  for (int i = 0; i < n; ++i) {
    L.a[i] = a[i];
    L.max_entries[i] = P[i].max_entries;
    pres_blocks = std::max<long long>(pres_blocks, ceil_div((long long)a[i].B * P[i].nunit * 64, 256));
    mask_blocks = std::max<long long>(mask_blocks, ceil_div((long long)P[i].max_entries, 4));
  }
  k_code_presence_legs<<<dim3((unsigned)pres_blocks, 1, n), 256, 0, s>>>(L);
  k_wg_plan_legs<<<dim3(1, 1, n), 1024, 0, s>>>(L);
  k_wg_masks_legs<<<dim3((unsigned)mask_blocks, 1, n), 256, 0, s>>>(L);
}

// a bf16 dW leg ready to run: its launch arguments over (plan, run workspace), the channel-sum
// buffer in that workspace and the output tile shape
struct WgRun {
  WgArgs a;
  float* csum;
  int fm;
};
static int wg_run(WgRun& r, const rgbd_dsam_dw_run& q) {
  const WgPlan P = wg_plan(q.B, q.Cin, q.h, q.w, q.Cout);
  RGBD_REQUIRE(wg_shape_ok(q.B, q.Cin, q.h, q.w, q.Cout, P), RGBD_E_SHAPE);
  r.a = wg_args(P, (char*)q.plan, q.ws, q.gout_nhwc, q.x_nhwc, q.code, q.B, q.Cin, q.h, q.w, q.Cout);
  r.csum = (float*)((char*)q.ws + dw_run_ws(wg_max_items(P) * q.Cout * 9 * q.Cin, q.B, q.Cout).csum);
  r.fm = P.fm;
  return RGBD_OK;
}

// One leg's GEMM in a launch of its own, with its bias channel sums: of the NCHW gradient when
// there is one (k_chan_sum), else of the NHWC one, drained by the GEMM's workgroups (fold)
static int wg_leg(const WgRun& r, const void* gout_nchw, hipStream_t s) {
  WgMulti<1> m;
  m.a[0] = r.a;
  m.csum[0] = r.csum;
  m.n = 1;
  m.fold = gout_nchw == nullptr;
  const hipError_t e = launch_wg_fm(r.fm, m, s);
  if (e != hipSuccess) return (int)e;
  if (gout_nchw)
    k_chan_sum<bf16_t><<<r.a.B * r.a.Cout, 256, 0, s>>>((const bf16_t*)gout_nchw, r.a.ho * r.a.wo, r.csum);
  return RGBD_OK;
}

static CombArgs comb_args(const WgRun& r, bool nchw_sums, const rgbd_decomp_info* info, const rgbd_dsam_dw_run& q) {
  CombArgs c;
  c.partial = r.a.partial;
  c.items = r.a.items;
  c.counts = r.a.counts;
  c.Cin = r.a.Cin;
  c.Cout = r.a.Cout;
  c.dconv_w = q.dconv_w;
  c.dproj_w = q.dproj_w;
  c.csum = r.csum;
  c.info = info;
  c.B = r.a.B;
  c.nsplit = nchw_sums ? 1 : chan_sum_splits(r.a.ho * r.a.wo);
  c.dbias = q.dbias;
  return c;
}

}  // namespace

namespace rgbd::k5 {

bool wgrad_shape_ok(int B, int Cin, int h, int w, int Cout) {
  return wg_shape_ok(B, Cin, h, w, Cout, wg_plan(B, Cin, h, w, Cout));
}
size_t wgrad_plan_bytes(int B, int Cin, int h, int w, int Cout) {
  return wg_plan_ws(wg_plan(B, Cin, h, w, Cout), B).total;
}
size_t wgrad_partial_elems(int B, int Cin, int h, int w, int Cout) {
  return wg_max_items(wg_plan(B, Cin, h, w, Cout)) * Cout * 9 * Cin;
}

int wgrad_plan(int n, const rgbd_dsam_leg* legs, hipStream_t s) {
  WgArgs a[WG_MAXLEG];
  WgPlan P[WG_MAXLEG];
  for (int i = 0; i < n; ++i) {
    const rgbd_dsam_leg& g = legs[i];
    P[i] = wg_plan(g.B, g.Cin, g.h, g.w, g.Cout);
    RGBD_REQUIRE(wg_shape_ok(g.B, g.Cin, g.h, g.w, g.Cout, P[i]), RGBD_E_SHAPE);
    a[i] = wg_args(P[i], (char*)g.plan, nullptr, nullptr, nullptr, g.code, g.B, g.Cin, g.h, g.w, g.Cout);
  }
  wg_plan_launch(n, a, P, s);
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

int wgrad_bf16(int n, const rgbd_dsam_dw_run* runs, const void* gout_nchw, const rgbd_decomp_info* info,
               hipStream_t s) {
  TimerScope ts("dsam_wgrad", s);
  WgRun r[2];
  for (int i = 0; i < n; ++i) {
    const int rc = wg_run(r[i], runs[i]);
    if (rc != RGBD_OK) return rc;
  }
  if (n == 2 && r[0].fm == r[1].fm) {  // one GEMM launch over both legs' work lists
    WgMulti<2> m;
    for (int i = 0; i < 2; ++i) {
      m.a[i] = r[i].a;
      m.csum[i] = r[i].csum;
    }
    m.n = 2;
    m.fold = 1;
    const hipError_t e = launch_wg_fm(r[0].fm, m, s);
    if (e != hipSuccess) return (int)e;
  } else {  // one leg, or tile shapes that differ: one launch per leg
    for (int i = 0; i < n; ++i) {
      const int rc = wg_leg(r[i], gout_nchw, s);
      if (rc != RGBD_OK) return rc;
    }
  }
  // the combine of the item partials into the reference filters (it also writes the bias
  // gradients), all legs in one launch
  CombArgs c[2];
  int cin = 0, cout = 0;
  for (int i = 0; i < n; ++i) {
    c[i] = comb_args(r[i], gout_nchw != nullptr, info, runs[i]);
    cin = std::max(cin, c[i].Cin);
    cout = std::max(cout, c[i].Cout);
  }
  k_dsam_wgrad_fold<<<dim3(cin / FOLD_C, cout, n), FOLD_T, 0, s>>>(c[0], c[n - 1]);
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

}  // namespace rgbd::k5

