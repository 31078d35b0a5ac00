// K5, bf16 forward / dX: the code-merged masked convolution as a persistent LDS-DMA MFMA kernel
// (k_dsam_lds) over a device-built plan (k_dsam_plan, k_dsam_items).  The host plan arithmetic and
// the launch functions (dsam_common.hpp) follow the kernels; the diagnostic build's stamp state
// and its rgbd_debug_dsam_* entry points are at the end.
#include "dsam_common.hpp"

using namespace rgbd;
using namespace rgbd::k5;

namespace {

// The masked sum  sum_i conv_i(x * m_i) + proj(x)  is regrouped by region CODE (the 4-bit
// pooled mask pattern of a source pixel, bit i = m_i): a source pixel with code k meets the
// merged filter  W_k = proj + sum_{i in k} conv_i  (packed per code by k_pack_codes, dsam_pack.hip), so
// each im2col row is multiplied by ONE filter instead of popcount(k) + 1 of them.  Rows are
// output pixels flattened over batch x grid (forward) or over one stride-2 parity class of the
// input grid (dX, where only the taps of that class are live).

// Code-merged masked conv, bf16 (fwd and dX).  Workgroup = 8 waves (2 along M x 4 along N),
// tile 8 x 16 output pixels (128 rows) x 192 columns, wave tile 64 x 48 (4 x 3 MFMA 16x16x32).
// Steps run over (tap, group of KC 32-channel chunks, region code present among the tile's
// rows at that tap); each step's operands arrive by LDS-DMA in an S-stage ring, S-1 steps ahead:
//   A  the 128 im2col rows x KC*64 B (a row whose tap falls outside the input re-reads an
//      in-bounds pixel of its own row; rows whose code differs from the step's code, or whose
//      tap is outside, are zeroed in registers after the fragment read);
//   B  the KC contiguous 192-row x 64-B tiles of the packed W_code (k_pack_codes' wfwd /
//      wbwd layout): linear copies.
// Load balance: a tile's step count is 9 x (codes per tap) x chunk groups, 1x..5x a dense tile
// on real scenes (region boundaries), so k_dsam_plan records each tile's per-tap code sets
// and the tile's steps are cut into nc = ceil(steps / chunk_len) equal chunks, one workgroup
// each; the last chunk of a multi-chunk tile to finish sums the f32 partials in chunk order.
constexpr int LD_BM = 128, LD_BN = 192, LD_CH = 8;  // tile rows, tile columns, max chunks per tile
constexpr int LD_MAXSTEP = 2048;    // steps of one tile (9 taps x 16 codes x chunk groups)
constexpr int LD_A1 = LD_BM * 64;   // 8 KB per chunk
constexpr int LD_B1 = LD_BN * 64;   // 12 KB per chunk
template <int KC>
struct LdCfg {
  static constexpr int S = KC == 3 ? 2 : (KC == 2 ? 3 : 6);  // ring depth the LDS admits
  static constexpr int A = KC * LD_A1;
  static constexpr int STAGE = KC * (LD_A1 + LD_B1);
  static constexpr int ROWTAB = S * STAGE;                // [128] int4 row table
  static constexpr int ROWOUT = ROWTAB + LD_BM * 16;      // [128] int4 NCHW base, NHWC pixel, n_masks
  static constexpr int TMASK = ROWOUT + LD_BM * 16;       // [9] u32 code set per tap, [9][16] u8 code list
  static constexpr int BSUM = TMASK + 64 + 160;           // [5][192] f32 bias prefix sums
  static constexpr int STEPTAB = BSUM + 5 * LD_BN * 4;    // [LD_MAXSTEP] int: tap | cg << 4 | code << 12
  static constexpr size_t SMEM = STEPTAB + LD_MAXSTEP * 4;
  static_assert(SMEM <= 163840, "LDS budget");
};
constexpr int LD_EPI_LD = LD_BM + 4;  // epilogue LDS tile [96 n][132] f32 (two halves)

struct LdGeom {
  int py, px, Hc, Wc, nyl, nxl, ntap, tiles_x, tiles_y, ntiles;
};
__device__ __forceinline__ LdGeom ld_geom(const ConvArgs& a, int cls) {
  LdGeom G;
  G.py = G.px = 0;
  G.Hc = a.Ho;
  G.Wc = a.Wo;
  if (a.transposed) {
    G.py = cls >> 1;
    G.px = cls & 1;
    G.Hc = (a.Ho - G.py + 1) >> 1;
    G.Wc = (a.Wo - G.px + 1) >> 1;
  }
  G.nyl = a.transposed ? (G.py ? 2 : 1) : 3;
  G.nxl = a.transposed ? (G.px ? 2 : 1) : 3;
  G.ntap = G.nyl * G.nxl;
  G.tiles_x = (G.Wc + 15) >> 4;
  G.tiles_y = (G.Hc + 7) >> 3;
  G.ntiles = a.linear ? (int)(((long long)a.B * G.Hc * G.Wc + LD_BM - 1) / LD_BM) : a.B * G.tiles_x * G.tiles_y;
  return G;
}
// live tap t of the class -> kernel tap (ky, kx) and source offset (dy, dx) from the row origin
__device__ __forceinline__ void ld_tap(const ConvArgs& a, const LdGeom& G, int t, int& ky, int& kx, int& dy,
                                       int& dx) {
  const int iy = t / G.nxl, ix = t - iy * G.nxl;
  if (a.transposed) {
    ky = G.py ? 2 * iy : 1;
    kx = G.px ? 2 * ix : 1;
    dy = (G.py + 1 - ky) >> 1;
    dx = (G.px + 1 - kx) >> 1;
  } else {
    ky = dy = iy;
    kx = dx = ix;
  }
}
// Row ml of tile `tile`: pixel (ty*8 + ml/16, tx*16 + ml%16) of the class grid.  Returns whether
// the row exists; org = origin pixel of its taps, rv = in-bounds taps, lo/hi = 4-bit code per tap.
__device__ __forceinline__ bool ld_row(const ConvArgs& a, const LdGeom& G, int tile, int ml, int& b, int& i,
                                       int& j, int& org, uint32_t& rv, uint32_t& lo, uint32_t& hi) {
  int iq, jq;
  if (a.linear) {  // row ml = pixel tile * 128 + ml of the batch's (class) grid
    const int hw = G.Hc * G.Wc, m = tile * LD_BM + ml;
    b = m / hw;
    const int rem = m - b * hw;
    iq = rem / G.Wc;
    jq = rem - iq * G.Wc;
  } else {
    b = tile / (G.tiles_x * G.tiles_y);
    const int trem = tile - b * G.tiles_x * G.tiles_y;
    iq = (trem / G.tiles_x) * 8 + (ml >> 4);
    jq = (trem % G.tiles_x) * 16 + (ml & 15);
  }
  const bool mv = b < a.B && iq < G.Hc && jq < G.Wc;
  b = mv ? b : 0;
  i = mv ? iq : 0;
  j = mv ? jq : 0;
  rv = lo = hi = 0u;
  uint32_t cv[9];
  if (a.transposed) {
    const uint32_t rc = a.code[((long long)b * a.Ho + 2 * i + G.py) * a.Wo + 2 * j + G.px];
    org = mv ? (b * a.Hi + i) * a.Wi + j : 0;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      int ky, kx, dy, dx;
      ld_tap(a, G, t < G.ntap ? t : 0, ky, kx, dy, dx);
      if (mv && t < G.ntap && i + dy < a.Hi && j + dx < a.Wi) rv |= 1u << t;
      cv[t] = rc;
    }
  } else {
    org = mv ? (b * a.Hi + 2 * i - 1) * a.Wi + 2 * j - 1 : 0;
    int off[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int iy = 2 * i - 1 + t / 3, ix = 2 * j - 1 + t % 3;
      const bool inb = mv && iy >= 0 && iy < a.Hi && ix >= 0 && ix < a.Wi;
      if (inb) rv |= 1u << t;
      off[t] = inb ? org + (t / 3) * a.Wi + t % 3 : 0;
    }
#pragma unroll
    for (int t = 0; t < 9; ++t) cv[t] = a.code[off[t]];
  }
#pragma unroll
  for (int t = 0; t < 9; ++t)
    if ((rv >> t) & 1u) {
      const uint32_t c = cv[t] & 15u;
      if (t < 8) lo |= c << (4 * t); else hi |= c;
    }
  return mv;
}
__device__ __forceinline__ int ld_steps(const uint16_t* tm, int ntap, int ncg) {
  int s = 0;
  for (int t = 0; t < ntap; ++t) s += __popc((uint32_t)tm[t]) * ncg;
  return s;
}
__device__ __forceinline__ int ld_nchunks(int steps, int len) {
  const int n = (steps + len - 1) / len;
  return n < 1 ? 1 : (n > LD_CH ? LD_CH : n);
}

// Plan: per (class, tile) the set of region codes the tile's rows meet at each live tap,
// tmasks[(cls * ntiles0 + tile) * 16 + t] (u16).  One 128-thread workgroup per tile.
__device__ __forceinline__ void plan_tile(const ConvArgs& a, int cls, int tile, int ntn) {
  __shared__ uint32_t tm_s[9];
  const int ntiles0 = a.ntiles0, tid = threadIdx.x;
  const LdGeom G = ld_geom(a, cls);
  if (tile >= G.ntiles) return;
  if (tid < 9) tm_s[tid] = 0u;
  __syncthreads();
  int b, i, j, org;
  uint32_t rv, lo, hi;
  ld_row(a, G, tile, tid, b, i, j, org, rv, lo, hi);
  uint32_t tm[5] = {0u, 0u, 0u, 0u, 0u};
#pragma unroll
  for (int t = 0; t < 9; ++t)
    if ((rv >> t) & 1u) {
      const uint32_t c = (t < 8 ? lo >> (4 * t) : hi) & 15u;
      tm[t >> 1] |= (1u << c) << (16 * (t & 1));
    }
#pragma unroll
  for (int q = 0; q < 5; ++q)
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) tm[q] |= (uint32_t)__shfl_xor((int)tm[q], o);
  if ((tid & 63) == 0)
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const uint32_t v = (tm[t >> 1] >> (16 * (t & 1))) & 0xffffu;
      if (v) atomicOr(&tm_s[t], v);
    }
  __syncthreads();
  if (tid < 16) a.tmasks[((long long)cls * ntiles0 + tile) * 16 + tid] = tid < 9 ? (uint16_t)tm_s[tid] : 0;
  if (cls == 0 && tile == 0 && tid < LD_ZERO_BYTES / 16)
    reinterpret_cast<uint4*>(const_cast<bf16_t*>(a.zero))[tid] = make_uint4(0u, 0u, 0u, 0u);
  for (int q = tid; q < ntn; q += 128) a.tickets[((long long)cls * ntiles0 + tile) * ntn + q] = 0;
  if (cls == 0 && tile == 0 && tid < ntn) a.work[tid] = 0;
}

// Several conv legs planned by one launch (the forward cascade's three DSAMs and the two dX
// legs, right after the decomposition): blockIdx.z runs over (leg, class), blockIdx.x over tiles.
struct PlanLegs {
  ConvArgs a[PLAN_MAXLEG];
  int zb[PLAN_MAXLEG + 1];  // first z of each leg
  int ntn[PLAN_MAXLEG];
  int n;
};
__global__ __launch_bounds__(128) void k_dsam_plan(const PlanLegs L) {
  const int z = blockIdx.z;
  int leg = 0;
  while (leg + 1 < L.n && z >= L.zb[leg + 1]) ++leg;
  plan_tile(L.a[leg], z - L.zb[leg], blockIdx.x, L.ntn[leg]);
}

// Work list: per (class, tile) the chunk count, compacted into items (cls | chunk << 2 |
// tile << 5) in (class, tile, chunk) order by one workgroup; a[*nitems] = count.  dX lists the
// parity classes by decreasing live-tap count (3: 4 taps, 1 and 2: 2, 0: 1), so the longest
// items are taken first under the dynamic assignment.
__device__ __forceinline__ void items_body(const ConvArgs& a) {
  __shared__ int wsum[16];
  __shared__ int base_s;
  const int ntiles0 = a.ntiles0, ncg = a.ncg;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nclass = a.transposed ? 4 : 1, total = nclass * ntiles0;
  if (tid == 0) base_s = 0;
  __syncthreads();
  for (int e0 = 0; e0 < total; e0 += 1024) {
    const int e = e0 + tid;
    int nc = 0;
    if (e < total) {
      const int ce = e / ntiles0, tile = e - ce * ntiles0;
      const int cls = a.transposed ? (0x0213 >> (4 * ce)) & 15 : ce;  // class order 3, 1, 2, 0
      const LdGeom G = ld_geom(a, cls);
      if (tile < G.ntiles)
        nc = ld_nchunks(ld_steps(a.tmasks + ((long long)cls * ntiles0 + tile) * 16, G.ntap, ncg), a.chunk_len);
    }
    // block exclusive scan of nc
    int x = nc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(x, o);
      if (lane >= o) x += y;
    }
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    int before = base_s;
    for (int q = 0; q < w; ++q) before += wsum[q];
    const int off = before + x - nc;
    if (e < total) {
      const int ce = e / ntiles0, tile = e - ce * ntiles0;
      const int cls = a.transposed ? (0x0213 >> (4 * ce)) & 15 : ce;  // class order 3, 1, 2, 0
      for (int c = 0; c < nc; ++c) a.items[off + c] = cls | (c << 2) | (tile << 5);
    }
    __syncthreads();
    if (tid == 1023) base_s = off + nc;
    __syncthreads();
  }
  if (tid == 0) *a.nitems = base_s;
}
__global__ __launch_bounds__(1024) void k_dsam_items(const PlanLegs L) { items_body(L.a[blockIdx.x]); }

// Diagnostics (rgbd_debug_dsam_stamps): the STAMPS instantiation of k_dsam_lds has wave 0 of every
// workgroup record, for its first LD_STAMP_ITEMS items, s_memtime at: item taken, prologue tables
// built, first DMA landed, K loop done, partial hand-off done (or the early return of a non-last
// chunk), epilogue done; then the item's steps | chunks << 16 | chunk << 24 and the item word:
// stamps[(wg * LD_STAMP_ITEMS + k) * 8 + field].  The production instantiation has none of it.
constexpr int LD_STAMP_ITEMS = 4;
__device__ __forceinline__ void ld_stamp(unsigned long long* st, int f) {
  if (!st) return;
  __builtin_amdgcn_sched_barrier(0);
  const unsigned long long t = __builtin_amdgcn_s_memtime();
  if (threadIdx.x == 0) st[f] = t;
  __builtin_amdgcn_sched_barrier(0);
}

// NODMA (diagnostic build only, rgbd_debug_dsam_mode; timing only, the results are garbage):
// bit 0 drops the in-loop B copies, bit 1 the in-loop A copies, bit 2 the per-step barrier (each
// wave still waits for its own copies), bit 3 the fragment reads (constant MFMA operands); bit 5
// copies every step's weights from its code's first filter tile and bit 6 every step's input rows from
// one fixed pixel block (the copies stay, their sources become L2-resident: the ceiling of
// locality work).
// One (tile, chunk) item of k_dsam_lds for N tile ntile (of ntn).
template <int KC, int NODMA = 0, bool F32IO = false>
__device__ __forceinline__ void ld_item(const ConvArgs& a, int cls, int tile, int chunk, int ntile, int ntn,
                                        int* next_s, int nitems, unsigned long long* st = nullptr) {
  using Cfg = LdCfg<KC>;
  constexpr int S = Cfg::S;
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  int4* rowtab = (int4*)(smem + Cfg::ROWTAB);
  int4* rowout = (int4*)(smem + Cfg::ROWOUT);
  float* bsum = (float*)(smem + Cfg::BSUM);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int wm = wave & 1, wn = wave >> 1;
  const LdGeom G = ld_geom(a, cls);
  const int ncg = a.C / (32 * KC);  // chunk groups
  const uint16_t* tmg = a.tmasks + ((long long)cls * a.ntiles0 + tile) * 16;
  // the tile's 16 u16 code sets in two 16-byte loads (one round trip; per-element loads behind
  // `t < ntap` were nine serialized ones, most of the item's table time)
  uint32_t tmask[9];
  {
    const uint4 q0 = reinterpret_cast<const uint4*>(tmg)[0], q1 = reinterpret_cast<const uint4*>(tmg)[1];
    const uint32_t w[5] = {q0.x, q0.y, q0.z, q0.w, q1.x};
#pragma unroll
    for (int t = 0; t < 9; ++t) tmask[t] = t < G.ntap ? (w[t >> 1] >> (16 * (t & 1))) & 0xffffu : 0u;
  }
  int tb[10];
  tb[0] = 0;
#pragma unroll
  for (int t = 0; t < 9; ++t) tb[t + 1] = tb[t] + __popc(tmask[t]) * ncg;
  const int total = tb[9];
  const int nc = ld_nchunks(total, a.chunk_len);
  const int n0 = ntile * LD_BN;
  const bf16_t* xp = (const bf16_t*)a.x;
  const bf16_t* wp = (const bf16_t*)a.w;
  const uint32_t lds0 = (uint32_t)(uintptr_t)smem;
  // ---- prologue: row table (threads 0..127), code lists per tap (the N tile's bias prefix sums
  // were built once per workgroup by k_dsam_lds)
  // step table, tap major, then chunk group, then code (ascending): one thread per (tap, chunk
  // group) writes its run from registers (no LDS round trips)
  for (int q = tid; q < G.ntap * ncg; q += 512) {
    const int t = q / ncg, cg = q - t * ncg;
    uint32_t msk = 0u;
    int e = 0;
#pragma unroll
    for (int u = 0; u < 9; ++u) {
      if (u == t) msk = tmask[u];
      if (u < t) e += __popc(tmask[u]) * ncg;
    }
    e += cg * __popc(msk);
    int* steptab = (int*)(smem + Cfg::STEPTAB);
    while (msk) {
      steptab[e++] = t | (cg << 4) | ((__ffs(msk) - 1) << 12);
      msk &= msk - 1u;
    }
  }
  if (tid < LD_BM) {
    int b, i, j, org;
    uint32_t rv, lo, hi;
    const bool mv = ld_row(a, G, tile, tid, b, i, j, org, rv, lo, hi);
    rowtab[tid] = make_int4(org, (int)rv, (int)lo, (int)hi);
    int obase = -1, opix = 0, nmk = 0;
    if (mv) {
      const int oy = a.transposed ? 2 * i + G.py : i, ox = a.transposed ? 2 * j + G.px : j;
      opix = (b * a.Ho + oy) * a.Wo + ox;
      obase = (b * a.N * a.Ho + oy) * a.Wo + ox;
      nmk = a.info ? a.info[b].n_masks : 0;
    }
    rowout[tid] = make_int4(obase, opix, nmk, 0);
  }
  __syncthreads();
  ld_stamp(st, 1);
  // DMA role: A rows 16*wave + lane/4 of every chunk, slot lane%4.  A row that is outside the
  // input at the step's tap, or whose source code is not the step's code, is read from the zero
  // row instead: it contributes exactly zero, with no masking of fragments in registers.
  const int R = 16 * wave + (lane >> 2);
  int aorg, achk;
  uint32_t aval, alo, ahi;
  {
    const int4 e = rowtab[R];
    aorg = e.x;
    aval = (uint32_t)e.y;
    alo = (uint32_t)e.z;
    ahi = (uint32_t)e.w;
    achk = 8 * ((lane & 3) ^ lds_swz(R));
  }
  const int* steptab = (const int*)(smem + Cfg::STEPTAB);
  const bf16_t* zrow = a.zero + achk;
  const int s0 = (int)((long long)chunk * total / nc), s1 = (int)((long long)(chunk + 1) * total / nc);
  const int nst = s1 - s0;
  if (st && threadIdx.x == 0) st[6] = (unsigned long long)(nst | (nc << 16) | (chunk << 24));
  auto issue = [&](int slot, int s, bool inloop = false) {  // step s (absolute)
    const int e = __builtin_amdgcn_readfirstlane(steptab[s]);
    const int t = e & 15, cg = (e >> 4) & 255, code = e >> 12;
    int ky, kx, dy, dx;
    ld_tap(a, G, t, ky, kx, dy, dx);
    const int delta = dy * a.Wi + dx, tap = ky * 3 + kx;
    const uint32_t sb = lds0 + slot * Cfg::STAGE;
    const uint32_t rc = (t < 8 ? alo >> (4 * t) : ahi) & 15u;
    const bool live = ((aval >> t) & 1u) && rc == (uint32_t)code;
    const bf16_t* asrc = live ? xp + (long long)(aorg + delta) * a.C + cg * 32 * KC + achk : zrow;
    if constexpr ((NODMA & 64) != 0)  // timing only: every step's rows from one fixed 128-pixel block
      if (inloop) asrc = xp + (long long)R * a.C + achk;
    if (!((NODMA & 2) && inloop))
#pragma unroll
      for (int kc = 0; kc < KC; ++kc) dma_lds16(live ? asrc + kc * 32 : zrow, sb + kc * LD_A1 + wave * 1024);
    if ((NODMA & 1) && inloop) return;
    const long long tstride = (long long)a.N * 32;  // one (code, tap, chunk) tile, elements
    const bf16_t* bsrc = wp + ((long long)(code * 9 + tap) * (a.C / 32) + cg * KC) * tstride + (long long)n0 * 32 + lane * 8;
    if constexpr ((NODMA & 32) != 0)  // timing only: every step's weights from its code's first tile
      if (inloop) bsrc = wp + (long long)(code * 9) * (a.C / 32) * tstride + (long long)n0 * 32 + lane * 8;
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) {
      const bf16_t* tbk = bsrc + kc * tstride;
      const uint32_t db = sb + Cfg::A + kc * LD_B1;
      dma_lds16(tbk + wave * 512, db + wave * 1024);
      if (wave < 4) dma_lds16(tbk + (wave + 8) * 512, db + (wave + 8) * 1024);
    }
  };
  const int cnt = KC * (wave < 4 ? 3 : 2);  // DMA instructions of this wave per step
  f32x4 acc[4][3];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int nj = 0; nj < 3; ++nj) acc[mi][nj] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int npro = nst < S - 1 ? nst : S - 1;
  for (int i = 0; i < npro; ++i) issue(i, s0 + i);
  if (npro >= 2) vm_wait_barrier_dyn((npro - 1) * cnt);  // step 0 landed, later ones may fly
  else vm_wait_barrier<0>();
  ld_stamp(st, 2);
#pragma unroll 1
  for (int s = 0; s < nst; ++s) {
    if (s + S - 1 < nst) issue((s + S - 1) % S, s0 + s + S - 1, true);
    const char* sa = smem + (s % S) * Cfg::STAGE;
    // fragments of chunk kc+1 are read while chunk kc's 12 MFMAs run
    Frag<bf16_t> fa[2][4], fb[2][3];
    auto rd = [&](int kc, int q) {
      if constexpr (NODMA & 8) {
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) fa[q][mi].v = make_uint4(lane, kc, s, mi);
#pragma unroll
        for (int nj = 0; nj < 3; ++nj) fb[q][nj].v = make_uint4(nj, lane, kc, s);
        return;
      }
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) {
        const int row = wm * 64 + 16 * mi + r;
        fa[q][mi].v = *reinterpret_cast<const uint4*>(sa + kc * LD_A1 + row * 64 + 16 * (g ^ lds_swz(row)));
      }
#pragma unroll
      for (int nj = 0; nj < 3; ++nj) {
        const int row = wn * 48 + 16 * nj + r;
        fb[q][nj].v = *reinterpret_cast<const uint4*>(sa + Cfg::A + kc * LD_B1 + row * 64 + 16 * (g ^ lds_swz(row)));
      }
    };
    rd(0, 0);
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) {
      if (kc + 1 < KC) rd(kc + 1, (kc + 1) & 1);
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int nj = 0; nj < 3; ++nj) mma(acc[mi][nj], fa[kc & 1][mi], fb[kc & 1][nj]);
    }
    // own DMA of step s+1 landed (only later steps' may stay in flight), LDS reads done, barrier
    const int ahead = (nst - 1 < s + S - 1 ? nst - 1 : s + S - 1) - (s + 1);
    if constexpr (NODMA & 4) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    else if (ahead <= 0) vm_wait_barrier<0>();
    else vm_wait_barrier_dyn(ahead * cnt);
  }
  ld_stamp(st, 3);
  // the workgroup's next item, taken now so the counter and work-list reads overlap the hand-off
  // and the epilogue; published in LDS at every exit (k_dsam_lds's barrier orders it)
  int nxt = 0, nxv = 0;
  bool have = false;
  if (tid == 0) nxt = __hip_atomic_fetch_add(a.work + ntile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  auto fetch_word = [&] {  // the next item's work-list word (waits for the counter)
    if (tid == 0 && !have) {
      nxv = nxt < nitems ? a.items[nxt] : 0;
      have = true;
    }
  };
  auto publish = [&] {
    fetch_word();
    if (tid == 0) {
      next_s[0] = nxt;
      next_s[1] = nxv;
    }
  };
  if (nc > 1) {
    // Multi-chunk tile: publish this chunk's fragment-native partial ([wave][mi][nj][lane][4] f32),
    // take a ticket; the chunk that draws nc-1 sums all partials in chunk order (deterministic)
    // and runs the epilogue.  The hand-off is write-through: every partial byte is stored and
    // loaded sc1 (16 B per lane, through one wave-uniform buffer descriptor), every storing wave
    // drains, one lane per workgroup adds to the tile's ticket after the barrier, and only the
    // workgroup whose add returned nc-1 loads (MI355X_MICROARCH.md, visibility table row 1;
    // cdna_hip_programming.md Guideline 16).  No agent-scope release (an XCD-wide L2 write-back)
    // or acquire is needed, and the result is correct for any placement of the chunks.
    const long long tslab = (((long long)cls * a.ntiles0 + tile) * ntn + ntile) * LD_CH;
    const __amdgpu_buffer_rsrc_t prs = wt_rsrc(a.partial + tslab * (LD_BN * LD_BM), LD_CH * LD_BN * LD_BM * 4);
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int nj = 0; nj < 3; ++nj)
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc[mi][nj]), prs,
                                               (chunk * (LD_BN * LD_BM) + (((wave * 4 + mi) * 3 + nj) * 64 + lane) * 4) * 4,
                                               0, WT_SC1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int* last_s = (int*)(smem + Cfg::TMASK);
    if (tid == 0) {
      const int old = __hip_atomic_fetch_add(a.tickets + tslab / LD_CH, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      *last_s = old == nc - 1;
    }
    __syncthreads();
    if (!*last_s) {
      ld_stamp(st, 4);
      publish();
      return;
    }
    // every partial of the tile in flight at once, then summed in chunk order
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int nj = 0; nj < 3; ++nj) acc[mi][nj] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < nc; ++c) {
      u32x4 pv[4][3];
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int nj = 0; nj < 3; ++nj)
          pv[mi][nj] = __builtin_amdgcn_raw_buffer_load_b128(
              prs, (c * (LD_BN * LD_BM) + (((wave * 4 + mi) * 3 + nj) * 64 + lane) * 4) * 4, 0, WT_SC1);
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int nj = 0; nj < 3; ++nj) acc[mi][nj] += __builtin_bit_cast(f32x4, pv[mi][nj]);
    }
  }
  ld_stamp(st, 4);
  // ---- epilogue (same contract as k_conv_igemm), staged through LDS in two 96-column halves:
  // pass 1 runs along pixels (NCHW residual loads and stores), pass 2 along channels (NHWC);
  // every thread's loads of a pass are independent and issued together.
  if constexpr (F32IO) {
    // NHWC-only epilogue with a float32 interface (the forward cascade of the float32-interface
    // mode): the one-pass epilogue below with the residual read as float32 (two 16-byte loads
    // per item, all twelve of a thread in flight across the LDS staging) and res + (acc + bias)
    // stored twice: as float32 (two 16-byte stores: cp1 as the DGGM pass and the outputs take it)
    // and rounded once to bf16 (the next DSAM's operand).  Either store may be absent.
    constexpr int LDE = LD_BN + 4;
    constexpr int NCH = LD_BN / 8;
    constexpr int NIT = LD_BM * NCH / 512;
    static_assert(LD_BM * LDE * 4 <= Cfg::ROWTAB, "epilogue image must not overlap the row tables");
    float* et = (float*)smem;
    const float* rf = a.residual_f32_nhwc;
    float* of = a.out_f32_nhwc;
    bf16_t* onhwc = (bf16_t*)a.out_nhwc;
    float4 rv[NIT][2];
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int it = tid + 512 * i, ml = it / NCH, n = n0 + 8 * (it % NCH);
      const int4 ro = rowout[ml];
      rv[i][0] = rv[i][1] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (rf && ro.x >= 0 && n < a.N) {
        const float* rp = rf + (long long)ro.y * a.N + n;
        rv[i][0] = *reinterpret_cast<const float4*>(rp);
        rv[i][1] = *reinterpret_cast<const float4*>(rp + 4);
      }
    }
    __syncthreads();  // ring reads done
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int nj = 0; nj < 3; ++nj)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
          et[(wm * 64 + 16 * mi + 4 * g + reg) * LDE + wn * 48 + 16 * nj + r] = acc[mi][nj][reg];
    __syncthreads();
    fetch_word();
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int it = tid + 512 * i, ml = it / NCH, nl = 8 * (it % NCH), n = n0 + nl;
      const int4 ro = rowout[ml];
      if (ro.x < 0 || n >= a.N) continue;
      const float4 e0 = *reinterpret_cast<const float4*>(et + ml * LDE + nl);
      const float4 e1 = *reinterpret_cast<const float4*>(et + ml * LDE + nl + 4);
      float v[8] = {e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w};
      const float rr[8] = {rv[i][0].x, rv[i][0].y, rv[i][0].z, rv[i][0].w, rv[i][1].x, rv[i][1].y, rv[i][1].z, rv[i][1].w};
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] += bsum[ro.z * LD_BN + nl + e];
      if (rf)
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = rr[e] + v[e];
      const long long o = (long long)ro.y * a.N + n;
      if (of) {
        *reinterpret_cast<float4*>(of + o) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(of + o + 4) = make_float4(v[4], v[5], v[6], v[7]);
      }
      if (onhwc)
        *reinterpret_cast<uint4*>(onhwc + o) =
            make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
    }
    ld_stamp(st, 5);
    publish();
    return;
  } else if (!a.out_nchw) {
    // NHWC-only epilogue (the hot path's forward cascade and dX): one pass.  The accumulators go
    // to an LDS image [128 rows][196] f32 (rows = tile pixels; the 4-float pad makes the 4 rows
    // a wave writes per register land on disjoint banks), then each thread owns 6 (row, 8-channel)
    // items: all six 16-byte NHWC residual loads in flight together, two 16-byte LDS reads, the
    // bias sum of the row's image, res + (acc + bias) rounded once, one 16-byte store.
    constexpr int LDE = LD_BN + 4;
    constexpr int NCH = LD_BN / 8;
    constexpr int NIT = LD_BM * NCH / 512;
    static_assert(LD_BM * LDE * 4 <= Cfg::ROWTAB, "epilogue image must not overlap the row tables");
    float* et = (float*)smem;
    const bf16_t* rnhwc = (const bf16_t*)a.residual_nhwc;
    bf16_t* onhwc = (bf16_t*)a.out_nhwc;
    uint4 rv[NIT];  // residual loads first: in flight while the accumulators go through LDS
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int it = tid + 512 * i, ml = it / NCH, n = n0 + 8 * (it % NCH);
      const int4 ro = rowout[ml];
      rv[i] = make_uint4(0u, 0u, 0u, 0u);
      if (rnhwc && ro.x >= 0 && n < a.N) rv[i] = *reinterpret_cast<const uint4*>(rnhwc + (long long)ro.y * a.N + n);
    }
    __syncthreads();  // ring reads done
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int nj = 0; nj < 3; ++nj)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
          et[(wm * 64 + 16 * mi + 4 * g + reg) * LDE + wn * 48 + 16 * nj + r] = acc[mi][nj][reg];
    __syncthreads();
    fetch_word();
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int it = tid + 512 * i, ml = it / NCH, nl = 8 * (it % NCH), n = n0 + nl;
      const int4 ro = rowout[ml];
      if (ro.x < 0 || n >= a.N) continue;
      const float4 e0 = *reinterpret_cast<const float4*>(et + ml * LDE + nl);
      const float4 e1 = *reinterpret_cast<const float4*>(et + ml * LDE + nl + 4);
      float v[8] = {e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w};
      const uint32_t uw[4] = {rv[i].x, rv[i].y, rv[i].z, rv[i].w};
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] += bsum[ro.z * LD_BN + nl + e];
      if (rnhwc)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[2 * e] = __uint_as_float(uw[e] << 16) + v[2 * e];
          v[2 * e + 1] = __uint_as_float(uw[e] & 0xffff0000u) + v[2 * e + 1];
        }
      *reinterpret_cast<uint4*>(onhwc + (long long)ro.y * a.N + n) =
          make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
    }
    ld_stamp(st, 5);
    publish();
    return;
  }
  float* et = (float*)smem;  // [96 n][LD_EPI_LD] f32
  const bf16_t* res = (const bf16_t*)a.residual;
  bf16_t* onchw = (bf16_t*)a.out_nchw;
  bf16_t* onhwc = (bf16_t*)a.out_nhwc;
  const long long HoWo = (long long)a.Ho * a.Wo;
  constexpr int HN = LD_BN / 2;
  for (int half = 0; half < 2; ++half) {
    __syncthreads();  // ring reads / previous half done
    if ((wn >> 1) == half)
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int nj = 0; nj < 3; ++nj)
#pragma unroll
          for (int reg = 0; reg < 4; ++reg)
            et[((wn & 1) * 48 + 16 * nj + r) * LD_EPI_LD + wm * 64 + 16 * mi + 4 * g + reg] = acc[mi][nj][reg];
    __syncthreads();
    const int nh = n0 + half * HN;
    if (onchw) {
    // pass 1: items (channel, 4 consecutive tile rows = 4 consecutive pixels of one tile row);
    // forward rows are contiguous in NCHW (8-byte residual loads / stores), dX rows are not
    constexpr int NQ = HN * LD_BM / 4 / 512;  // 6 items per thread
    float4 rq[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {  // residual loads, all in flight
      const int it = tid + 512 * q, nl = it / (LD_BM / 4), ml = (it % (LD_BM / 4)) * 4, n = nh + nl;
      rq[q] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (!res || n >= a.N) continue;
      const int4 r0 = rowout[ml], r3 = rowout[ml + 3];
      const long long o = r0.x + (long long)n * HoWo;
      if (!a.transposed && r0.x >= 0 && r3.x == r0.x + 3) {
        const uint2 u = *reinterpret_cast<const uint2*>(res + o);
        rq[q] = make_float4(bf16_to_f32((bf16_t)u.x), bf16_to_f32((bf16_t)(u.x >> 16)), bf16_to_f32((bf16_t)u.y),
                            bf16_to_f32((bf16_t)(u.y >> 16)));
      } else {
        float t4[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int4 re = rowout[ml + e];
          t4[e] = re.x >= 0 ? bf16_to_f32(res[re.x + (long long)n * HoWo]) : 0.f;
        }
        rq[q] = make_float4(t4[0], t4[1], t4[2], t4[3]);
      }
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int it = tid + 512 * q, nl = it / (LD_BM / 4), ml = (it % (LD_BM / 4)) * 4, n = nh + nl;
      if (n >= a.N) continue;
      const float rr[4] = {rq[q].x, rq[q].y, rq[q].z, rq[q].w};
      bf16_t tv[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int4 re = rowout[ml + e];
        float v = et[nl * LD_EPI_LD + ml + e] + bsum[re.z * LD_BN + half * HN + nl];
        if (res) v = rr[e] + v;
        tv[e] = f32_to_bf16(v);
        et[nl * LD_EPI_LD + ml + e] = bf16_to_f32(tv[e]);
      }
      if (onchw) {
        const int4 r0 = rowout[ml], r3 = rowout[ml + 3];
        if (!a.transposed && r0.x >= 0 && r3.x == r0.x + 3) {
          *reinterpret_cast<uint2*>(onchw + r0.x + (long long)n * HoWo) =
              make_uint2((uint32_t)tv[0] | ((uint32_t)tv[1] << 16), (uint32_t)tv[2] | ((uint32_t)tv[3] << 16));
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int4 re = rowout[ml + e];
            if (re.x >= 0) onchw[re.x + (long long)n * HoWo] = tv[e];
          }
        }
      }
    }
    }  // pass 1
    if (onhwc) {
      // pass 2: items (tile row, 8 consecutive channels) -> one 16-byte store.  Consecutive lanes
      // take consecutive tile rows of the same 8 channels, so the LDS column reads are
      // conflict-free.  Without pass 1 (no NCHW output: the bf16 dX of the hot path) the bias
      // and the NHWC residual are added here, in pass 1's order: res + (acc + bias), rounded once.
      __syncthreads();
      const bool fused = !onchw;
      const bf16_t* rnhwc = (const bf16_t*)a.residual_nhwc;
      for (int it = tid; it < LD_BM * (HN / 8); it += 512) {
        const int ml = it % LD_BM, nl = (it / LD_BM) * 8, n = nh + nl;
        const int4 ro = rowout[ml];
        if (ro.x < 0 || n >= a.N) continue;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = et[(nl + e) * LD_EPI_LD + ml];
        if (fused) {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] += bsum[ro.z * LD_BN + half * HN + nl + e];
          if (rnhwc) {
            const uint4 u = *reinterpret_cast<const uint4*>(rnhwc + (long long)ro.y * a.N + n);
            const uint32_t uw[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              v[2 * e] = __uint_as_float(uw[e] << 16) + v[2 * e];
              v[2 * e + 1] = __uint_as_float(uw[e] & 0xffff0000u) + v[2 * e + 1];
            }
          }
        }
        *reinterpret_cast<uint4*>(onhwc + (long long)ro.y * a.N + n) =
            make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
      }
    }
  }
  ld_stamp(st, 5);
  publish();
}

// Persistent: grid (workgroups, N tiles); each workgroup takes the next item of its N tile's list
// from a counter (items differ up to ~5x in steps: dynamic assignment balances the tail; the
// multi-chunk reductions stay in chunk order, so results do not depend on who ran what).
template <int KC, bool STAMPS = false, int NODMA = 0, bool F32IO = false>
__global__ __launch_bounds__(512, 1) void k_dsam_lds(ConvArgs a) {
  using Cfg = LdCfg<KC>;
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  if constexpr (NODMA != 0) {  // the ring starts zeroed: slots the modes never fill hold finite values
    for (int e = threadIdx.x; e < Cfg::S * Cfg::STAGE / 16; e += 512)
      reinterpret_cast<uint4*>(smem)[e] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
  }
  int* next_s = (int*)(smem + Cfg::TMASK + 216);  // free bytes behind the per-tap code lists: item, word
  const int nitems = *a.nitems;
  const int ntile = blockIdx.y;
  {  // the N tile's bias prefix sums over the four conv biases, kept for every item
    float* bsum = (float*)(smem + Cfg::BSUM);
    const int n0 = ntile * LD_BN;
    for (int e = threadIdx.x; e < 5 * LD_BN; e += 512) {
      const int k = e / LD_BN, nl = e - k * LD_BN, n = n0 + nl;
      float s = 0.f;
      if (a.bias4 && n < a.N)
        for (int sb = 0; sb < k; ++sb) s += a.bias4[sb * a.N + n];
      bsum[e] = s;
    }
  }
  if (threadIdx.x == 0) {
    const int it = __hip_atomic_fetch_add(a.work + ntile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    next_s[0] = it;
    next_s[1] = it < nitems ? a.items[it] : 0;
  }
  int done = 0;
  for (;;) {
    unsigned long long* st = nullptr;
    if constexpr (STAMPS) {
      if (done < LD_STAMP_ITEMS)
        st = a.stamps + ((long long)(blockIdx.x + blockIdx.y * gridDim.x) * LD_STAMP_ITEMS + done) * 8;
      ++done;
    }
    __syncthreads();  // next_s published (first item: above; later: by the previous item)
    const int it = next_s[0], v = next_s[1];
    if (it >= nitems) break;  // workgroup-uniform
    ld_stamp(st, 0);
    if (st && threadIdx.x == 0) st[7] = (unsigned long long)v;
    // next_s is rewritten only after the item's K loop, behind its prologue barrier
    ld_item<KC, NODMA, F32IO>(a, v & 3, v >> 5, (v >> 2) & 7, ntile, gridDim.y, next_s, nitems, st);
  }
}

// ------------------------------------------------------------------ host: plan arithmetic
// chunks per step: three where C allows (two-stage ring).  Two (three-stage ring) measured slower
// (round 4: 2 300 cycles per 64-channel step vs 2 840 per 96-channel step; K5 0.707 vs 0.676 ms):
// the step is bound by LDS traffic (fragment reads + DMA writes), not by the DMA latency
int ld_kc(int C) { return C % 96 == 0 ? 3 : (C % 64 == 0 ? 2 : 1); }
// k_dsam_lds tiling of a conv: tiles of the largest parity class, N tiles
// Linear tiles when 8 x 16 blocks would leave more than 15 % of the rows dead (the small grids:
// dsam1 / dsam2 outputs, their dX parity classes)
int ld_linear(int Hc, int Wc) {
  const long long blk = (long long)((Hc + 7) / 8 * 8) * ((Wc + 15) / 16 * 16);
  return (long long)Hc * Wc * 100 < 85 * blk;
}
struct LdPlan {
  int ntiles0, ntn, kc, chunk_len, linear;
  size_t tmask_bytes, items_bytes, ticket_bytes, partial_bytes;
};
LdPlan ld_plan(const ConvArgs& a) {
  LdPlan p;
  const int Hc0 = a.transposed ? (a.Ho + 1) / 2 : a.Ho, Wc0 = a.transposed ? (a.Wo + 1) / 2 : a.Wo;
  const int nclass = a.transposed ? 4 : 1;
  p.linear = ld_linear(Hc0, Wc0);
  p.ntiles0 = p.linear ? (int)(((long long)a.B * Hc0 * Wc0 + LD_BM - 1) / LD_BM) : a.B * ((Hc0 + 7) / 8) * ((Wc0 + 15) / 16);
  p.ntn = ceil_div(a.N, LD_BN);
  p.kc = ld_kc(a.C);
  // chunk length in steps: one dense tile (one code per tap); 60 % and 150 % measured slower
  // (K5 0.74 / 0.78 vs 0.71 ms per step, round 3)
  const int ntap = a.transposed ? 4 : 9;  // class 3 of dX has 4 live taps
  p.chunk_len = std::max(1, ntap * (a.C / (32 * p.kc)));
  p.tmask_bytes = align256((size_t)nclass * p.ntiles0 * 16 * sizeof(uint16_t));
  p.items_bytes = align256(((size_t)nclass * p.ntiles0 * LD_CH + 1) * sizeof(int));
  p.ticket_bytes = align256((size_t)(nclass * p.ntiles0 * p.ntn + 64) * sizeof(int)) + LD_ZERO_BYTES;  // + work counters
  p.partial_bytes = align256((size_t)nclass * p.ntiles0 * p.ntn * LD_CH * LD_BN * LD_BM * sizeof(float));
  return p;
}
size_t ld_plan_bytes(const LdPlan& p) { return p.tmask_bytes + p.items_bytes + p.ticket_bytes; }
// The bf16 launch arguments of a conv leg over its plan buffer [code sets | work list | tickets,
// counters, zero row] (ld_plan_bytes) and its partial-tile buffer (P.partial_bytes).
ConvArgs conv_carve(const ConvArgs& a, const LdPlan& P, char* plan, float* partial) {
  ConvArgs b = a;
  const int nclass = a.transposed ? 4 : 1;
  b.tmasks = (uint16_t*)plan;
  b.items = (int*)(plan + P.tmask_bytes);
  b.nitems = b.items + (size_t)nclass * P.ntiles0 * LD_CH;
  b.tickets = (int*)(plan + P.tmask_bytes + P.items_bytes);
  b.work = b.tickets + (size_t)nclass * P.ntiles0 * P.ntn;
  b.zero = (const bf16_t*)(plan + ld_plan_bytes(P) - LD_ZERO_BYTES);  // the ticket region's tail
  b.partial = partial;
  b.ntiles0 = P.ntiles0;
  b.chunk_len = P.chunk_len;
  b.ncg = a.C / (32 * P.kc);
  b.linear = P.linear;
  return b;
}
bool ld_shape_ok(const ConvArgs& a, const LdPlan& P) {
  return a.C % 32 == 0 && a.N % 32 == 0 && (long long)a.B * a.Hi * a.Wi < (1ll << 31) && conv_mmax(a) < (1ll << 31) &&
         P.ntn <= 64 && 9 * 16 * (a.C / (32 * P.kc)) <= LD_MAXSTEP;
}

// ------------------------------------------------------------------ host: launches
#ifdef RGBD_DIAG
// rgbd_debug_dsam_stamps (diagnostic build only): buffer, its capacity in launches, launches
// stamped so far
unsigned long long* g_ld_stamps = nullptr;
int g_ld_stamp_cap = 0, g_ld_stamp_n = 0;
int g_ld_mode = 0;  // rgbd_debug_dsam_mode: NODMA bits of the stamped KC = 3 instantiation
#endif
// one instantiation of k_dsam_lds: its dynamic-LDS attribute once, then the launch
template <int KC, bool STAMPS, int NODMA, bool F32IO>
hipError_t launch_ld(const ConvArgs& c, dim3 grid, hipStream_t s) {
  static const hipError_t attr = hipFuncSetAttribute((const void*)k_dsam_lds<KC, STAMPS, NODMA, F32IO>,
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)LdCfg<KC>::SMEM);
  if (attr != hipSuccess) return attr;
  k_dsam_lds<KC, STAMPS, NODMA, F32IO><<<grid, 512, LdCfg<KC>::SMEM, s>>>(c);
  return hipSuccess;
}
// The instantiation of a launch with KC chunks per step.  The float32-interface forward
// (ConvArgs::residual_f32_nhwc / out_f32_nhwc) is one of its own, so the plain one's code does not
// depend on it; the diagnostic build stamps the plain one's launches while a stamp buffer has room.
template <int KC>
hipError_t launch_ld_kc(const ConvArgs& b, bool f32io, dim3 grid, hipStream_t s) {
  if (f32io) return launch_ld<KC, false, 0, true>(b, grid, s);
#ifdef RGBD_DIAG
  if (g_ld_stamps && g_ld_stamp_n < g_ld_stamp_cap && grid.x * grid.y <= 256) {
    ConvArgs c = b;
    c.stamps = g_ld_stamps + (size_t)g_ld_stamp_n++ * 256 * LD_STAMP_ITEMS * 8;
    if constexpr (KC == 3) {
      switch (g_ld_mode) {
        case 1: return launch_ld<KC, true, 1, false>(c, grid, s);
        case 2: return launch_ld<KC, true, 2, false>(c, grid, s);
        case 3: return launch_ld<KC, true, 3, false>(c, grid, s);
        case 7: return launch_ld<KC, true, 7, false>(c, grid, s);
        case 15: return launch_ld<KC, true, 15, false>(c, grid, s);
        case 32: return launch_ld<KC, true, 32, false>(c, grid, s);
        case 64: return launch_ld<KC, true, 64, false>(c, grid, s);
        case 96: return launch_ld<KC, true, 96, false>(c, grid, s);
        case 8: return launch_ld<KC, true, 8, false>(c, grid, s);
        default: break;
      }
    }
    return launch_ld<KC, true, 0, false>(c, grid, s);
  }
#endif
  return launch_ld<KC, false, 0, false>(b, grid, s);
}

}  // namespace

namespace rgbd::k5 {

bool conv_shape_ok(const ConvArgs& a) { return ld_shape_ok(a, ld_plan(a)); }
size_t conv_plan_bytes(const ConvArgs& a) { return ld_plan_bytes(ld_plan(a)); }
size_t conv_partial_bytes(const ConvArgs& a) { return ld_plan(a).partial_bytes; }

// plan + work list of n conv legs (two launches)
int conv_plan(int n, const ConvArgs* legs, void* const* plans, hipStream_t s) {
  PlanLegs L = {};
  L.n = n;
  int z = 0, mt = 1;
  for (int i = 0; i < n; ++i) {
    const LdPlan P = ld_plan(legs[i]);
    RGBD_REQUIRE(ld_shape_ok(legs[i], P), RGBD_E_SHAPE);
    L.a[i] = conv_carve(legs[i], P, (char*)plans[i], nullptr);
    L.zb[i] = z;
    L.ntn[i] = P.ntn;
    z += legs[i].transposed ? 4 : 1;
    mt = std::max(mt, P.ntiles0);
  }
  L.zb[n] = z;
  k_dsam_plan<<<dim3(mt, 1, z), 128, 0, s>>>(L);
  k_dsam_items<<<n, 1024, 0, s>>>(L);
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

// One planned conv leg (forward or dX): the persistent kernel over the leg's plan and its
// partial-tile buffer a.partial
int conv_bf16(const ConvArgs& a, const void* plan, hipStream_t s) {
  TimerScope ts(a.transposed ? "dsam_dx" : "dsam_fwd", s);
  const LdPlan P = ld_plan(a);
  RGBD_REQUIRE(ld_shape_ok(a, P), RGBD_E_SHAPE);
  const ConvArgs b = conv_carve(a, P, (char*)plan, a.partial);
  dim3 grid(std::max(1, 256 / P.ntn), P.ntn, 1);  // persistent: one LDS-bound workgroup per CU over all N tiles
  const bool f32io = a.residual_f32_nhwc || a.out_f32_nhwc;
  const hipError_t e = P.kc == 3   ? launch_ld_kc<3>(b, f32io, grid, s)
                       : P.kc == 2 ? launch_ld_kc<2>(b, f32io, grid, s)
                                   : launch_ld_kc<1>(b, f32io, grid, s);
  if (e != hipSuccess) return (int)e;
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

}  // namespace rgbd::k5

#ifdef RGBD_DIAG
extern "C" {

int rgbd_debug_dsam_stamps(void* buf, int launches) {
  RGBD_REQUIRE(buf ? launches > 0 : launches == 0, RGBD_E_ARG);  // (NULL, 0) stops
  g_ld_stamps = (unsigned long long*)buf;
  g_ld_stamp_cap = buf ? launches : 0;
  g_ld_stamp_n = 0;
  return RGBD_OK;
}
int rgbd_debug_dsam_mode(int mode) {
  RGBD_REQUIRE(mode == 0 || mode == 1 || mode == 2 || mode == 3 || mode == 7 || mode == 8 || mode == 15 || mode == 32 ||
                   mode == 64 || mode == 96,
               RGBD_E_ARG);
  g_ld_mode = mode;
  return RGBD_OK;
}

}  // extern "C"
#endif
