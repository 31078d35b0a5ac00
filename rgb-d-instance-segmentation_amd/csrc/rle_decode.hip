// f7: compressed COCO RLE strings decoded on the device — the reading half of the
// reference's per-image JSON (mask2former/predictor.py:974-1065 _load_json_prediction_data over
// pycocotools.mask.decode; the C routines are maskApi.c rleFrString and rleDecode).
//
// Counts stage (k_rle_counts, one workgroup per mask, RLE_CHUNK characters per step, one per lane):
//   rleFrString: a character c - 48 carries 5 value bits, bit 0x20 = another group follows, bit 0x10
//   of the last group = sign.  A character without bit 0x20 terminates a count; the scan of the
//   terminator flags numbers the counts, and each terminator assembles its value from the groups
//   behind it (at most 13 for a 64-bit long; read back from memory, so a count that straddles two
//   steps needs no carry).  The delta coding cnts[i] = x[i] + cnts[i-2] (i > 2) is two stride-2
//   prefix sums — odd indices chain from 1, even ones from 2, cnts[0] stands alone — and one more
//   prefix sum gives the run ends E[i] (unsigned 32-bit: h w < 2^31).  Index, odd, even and E sums
//   carry from step to step in registers.  Per mask: the number of counts, a status (RLE_BAD_*)
//   and, where the mask has the target size, "has a set pixel" = an odd count above 0.
// Paint stage (k_rle_paint, pixel-centric): a lane owns 4 consecutive pixels of one destination
//   row.  For the masks of its file from last to first it takes the source pixel (identity, or the
//   Pillow NEAREST tables of pil_nearest.hpp), the column-major position p = sx h + sy, and the
//   run holding p by an upper-bound search over E (first E > p: zero-length runs, whose ends
//   repeat, are stepped over); the pixel is set iff that run's index is odd.  The first hit is the
//   answer i + 1 — the painter's order of the reference, later masks over earlier ones — and no hit
//   gives 0.  A mask's E sits in LDS while it fits.  No atomics: every pixel is written once by
//   one lane, so the map is bitwise repeatable.  Stack mode is the same kernel with one mask per
//   "file" and a uint8 0/1 output (pycocotools.mask.decode).
// k_rle_any_set: "has a set pixel after the resize" for the masks whose size differs from the
//   target — the early-out painter cannot know it — by a wave ballot and a plain store of 1.
// Bound: the searches (log2(n) dependent LDS reads per pixel and candidate mask); the map is
//   written once, 16 bytes per lane.
#include "common.hpp"
#include "pil_nearest.hpp"

namespace rgbd {
namespace {

constexpr int RLE_CHUNK = 256;        // characters per step of the counts stage = its block size
constexpr int RLE_MAX_GROUPS = 13;    // 5-bit groups of a 64-bit long
constexpr int RLE_LDS_COUNTS = 4096;  // run ends of one mask kept in LDS by the painter (16 KiB)
constexpr int RLE_BAD_COUNT = 1;      // a negative count (or one past 2^31 - 1)
constexpr int RLE_BAD_TOTAL = 2;      // the counts do not sum to h w
constexpr int RLE_BAD_GROUP = 4;      // the last group is truncated, or a count has more than 13 groups
constexpr int RLE_PX = 4;             // pixels per lane of the painter

typedef unsigned long long u64;

// meta (int32, the same words on the host and on the device):
//   offsets [N+1] | hw [N][2] | take [N] | slot [N] | resized [N] | ranges [B+1]
struct Meta {
  const int32_t *offsets, *hw, *take, *slot, *resized, *ranges;
};
__host__ __device__ inline Meta meta_of(const int32_t* m, int N) {
  Meta t;
  t.offsets = m;
  t.hw = m + (N + 1);
  t.take = t.hw + 2 * (size_t)N;
  t.slot = t.take + N;
  t.resized = t.slot + N;
  t.ranges = t.resized + N;
  return t;
}

// inclusive sum over the 256 lanes of a block (4 waves); total = the block's sum
template <typename T>
__device__ __forceinline__ T block_scan(T v, T* sh, T& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(v, o);
    if (lane >= o) v += t;
  }
  if (lane == 63) sh[wv] = v;
  __syncthreads();
  T add = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < RLE_CHUNK / 64; ++k) {
    const T s = sh[k];
    if (k < wv) add += s;
    tot += s;
  }
  __syncthreads();
  total = tot;
  return v + add;
}

__global__ __launch_bounds__(RLE_CHUNK) void k_rle_counts(const uint8_t* __restrict__ chars,
                                                           const int32_t* __restrict__ meta, int N, int H, int W,
                                                           uint32_t* __restrict__ ends, int32_t* __restrict__ info) {
  __shared__ u64 sh64[RLE_CHUNK / 64];
  __shared__ int sh32[RLE_CHUNK / 64];
  const int m = blockIdx.x, tid = threadIdx.x;
  const Meta mt = meta_of(meta, N);
  const int off = mt.offsets[m], L = mt.offsets[m + 1] - off;
  const int h = mt.hw[2 * m], w = mt.hw[2 * m + 1];
  const uint8_t* s = chars + off;
  uint32_t* E = ends + off;  // count i of this mask lands at character slot i (counts <= characters)
  int n_counts = 0;
  u64 c_odd = 0, c_even = 0, c_end = 0;
  int bad = 0, any_set = 0;
  for (int base = 0; base < L; base += RLE_CHUNK) {
    const int j = base + tid;
    const bool valid = j < L;
    const int c = valid ? (int)s[j] - 48 : 0;
    const bool term = valid && !(c & 0x20);
    u64 x = 0;
    if (term) {
      int g = 1;  // groups of this count: the characters behind it that announce another group
      while (g <= RLE_MAX_GROUPS && j - g >= 0 && (((int)s[j - g] - 48) & 0x20)) ++g;
      if (g > RLE_MAX_GROUPS) {
        bad |= RLE_BAD_GROUP;
        g = RLE_MAX_GROUPS;
      }
      for (int q = 0; q < g; ++q) x |= (u64)(((int)s[j - g + 1 + q] - 48) & 0x1f) << (5 * q);
      if ((c & 0x10) && 5 * g < 64) x |= ~(u64)0 << (5 * g);
    }
    if (valid && j == L - 1 && !term) bad |= RLE_BAD_GROUP;
    int n_term;
    const int i = n_counts + block_scan<int>(term ? 1 : 0, sh32, n_term) - 1;
    u64 t_odd, t_even, t_end;
    const u64 odd = c_odd + block_scan<u64>(term && (i & 1) ? x : 0, sh64, t_odd);
    const u64 even = c_even + block_scan<u64>(term && !(i & 1) && i >= 2 ? x : 0, sh64, t_even);
    const u64 cnt = !term ? 0 : (i == 0 ? x : ((i & 1) ? odd : even));
    if (cnt > 0x7fffffffull) bad |= RLE_BAD_COUNT;  // negative counts wrap to the top of the range
    if (term && (i & 1) && cnt > 0) any_set = 1;
    const u64 e = c_end + block_scan<u64>(cnt, sh64, t_end);
    if (term) E[i] = (uint32_t)e;
    n_counts += n_term;
    c_odd += t_odd;
    c_even += t_even;
    c_end += t_end;
  }
  if (c_end != (u64)h * (u64)w) bad |= RLE_BAD_TOTAL;
  int status = 0;
  for (int bit = 1; bit <= RLE_BAD_GROUP; bit <<= 1) status |= __syncthreads_or(bad & bit) ? bit : 0;
  any_set = __syncthreads_or(any_set);
  if (tid == 0) {
    info[4 * m + 0] = n_counts;
    info[4 * m + 1] = status;
    info[4 * m + 2] = (h == H && w == W && any_set) ? 1 : 0;  // a resized mask: k_rle_any_set decides
    info[4 * m + 3] = 0;
  }
}

// index tables of the masks whose size differs from the target: slot k = [H] rows | [W] columns
__global__ void k_rle_tables(const int32_t* __restrict__ meta, int N, int H, int W, int* __restrict__ tabs) {
  const int axis = threadIdx.x;
  if (axis > 1) return;
  const Meta mt = meta_of(meta, N);
  const int m = mt.resized[blockIdx.x];
  int* t = tabs + (size_t)blockIdx.x * (H + W);
  if (axis == 0)
    pil_nearest_walk(mt.hw[2 * m], H, t);
  else
    pil_nearest_walk(mt.hw[2 * m + 1], W, t + H);
}

// first index r in [0, n) with E[r] > p, n when there is none
template <typename P>
__device__ __forceinline__ int run_of(P E, int n, uint32_t p) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (E[mid] <= p)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_rle_any_set(const int32_t* __restrict__ meta, int N, int H, int W,
                                                      const uint32_t* __restrict__ ends,
                                                      const int* __restrict__ tabs, int32_t* __restrict__ info) {
  const Meta mt = meta_of(meta, N);
  const int k = blockIdx.y, m = mt.resized[k];
  if (info[4 * m + 1] != 0) return;
  const int n = info[4 * m + 0], h = mt.hw[2 * m];
  const uint32_t* E = ends + mt.offsets[m];
  const int* t = tabs + (size_t)k * (H + W);
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  bool set = false;
  if (q < (long long)H * W) {
    const int y = (int)(q / W), x = (int)(q % W);
    const uint32_t p = (uint32_t)t[H + x] * (uint32_t)h + (uint32_t)t[y];
    const int r = run_of(E, n, p);
    set = r < n && (r & 1);
  }
  if (__ballot(set) != 0 && (threadIdx.x & 63) == 0) info[4 * m + 2] = 1;
}

// STACK false: out int32 [B][H][W], grid (x, B); STACK true: out uint8 [N][H][W], grid (x, N)
template <bool STACK>
__global__ __launch_bounds__(256) void k_rle_paint(const int32_t* __restrict__ meta, int N, int H, int W,
                                                    const uint32_t* __restrict__ ends, const int* __restrict__ tabs,
                                                    const int32_t* __restrict__ info, void* __restrict__ out) {
  __shared__ uint32_t sE[RLE_LDS_COUNTS];
  const Meta mt = meta_of(meta, N);
  const int b = blockIdx.y, tid = threadIdx.x;
  const int lpr = (W + RLE_PX - 1) / RLE_PX;  // lanes per row
  const long long lane = (long long)blockIdx.x * 256 + tid;
  const int y = (int)(lane / lpr), x0 = (int)(lane % lpr) * RLE_PX;
  unsigned pend = 0;  // bit q: pixel x0 + q is inside the map and has no answer yet
  if (y < H)
    for (int q = 0; q < RLE_PX; ++q) pend |= (x0 + q < W) ? 1u << q : 0u;
  const unsigned mine = pend;
  int res[RLE_PX] = {0, 0, 0, 0};
  const int first = STACK ? b : mt.ranges[b], last = STACK ? b + 1 : mt.ranges[b + 1];
  for (int m = last - 1; m >= first; --m) {
    const int n = info[4 * m + 0];
    const bool part = info[4 * m + 1] == 0 && (STACK || (mt.take[m] != 0 && info[4 * m + 2] != 0));
    if (!part) continue;  // block-uniform
    if (!__syncthreads_or(pend != 0)) break;  // also: every lane is done with the previous mask's sE
    const uint32_t* E = ends + mt.offsets[m];
    const bool in_lds = n <= RLE_LDS_COUNTS;
    if (in_lds)
      for (int i = tid; i < n; i += 256) sE[i] = E[i];
    __syncthreads();
    if (!pend) continue;
    const int k = STACK ? -1 : mt.slot[m];
    const int h = mt.hw[2 * m];
    const int* t = tabs + (size_t)(k < 0 ? 0 : k) * (H + W);
    const uint32_t sy = k < 0 ? (uint32_t)y : (uint32_t)t[y];
#pragma unroll
    for (int q = 0; q < RLE_PX; ++q) {
      if (!(pend >> q & 1)) continue;
      const uint32_t sx = k < 0 ? (uint32_t)(x0 + q) : (uint32_t)t[H + x0 + q];
      const uint32_t p = sx * (uint32_t)h + sy;
      const int r = in_lds ? run_of((const uint32_t*)sE, n, p) : run_of(E, n, p);
      if (r < n && (r & 1)) {
        res[q] = STACK ? 1 : m - first + 1;
        pend &= ~(1u << q);
      }
    }
  }
  if (!mine) return;
  const long long at = ((long long)b * H + y) * W + x0;
  if (STACK) {
    uint8_t* o = (uint8_t*)out + at;
    if (W % RLE_PX == 0) {
      *(uchar4*)o = make_uchar4((uint8_t)res[0], (uint8_t)res[1], (uint8_t)res[2], (uint8_t)res[3]);
    } else {
      for (int q = 0; q < RLE_PX; ++q)
        if (mine >> q & 1) o[q] = (uint8_t)res[q];
    }
  } else {
    int32_t* o = (int32_t*)out + at;
    if (W % RLE_PX == 0) {
      *(int4*)o = make_int4(res[0], res[1], res[2], res[3]);
    } else {
      for (int q = 0; q < RLE_PX; ++q)
        if (mine >> q & 1) o[q] = res[q];
    }
  }
}

// host-side validation of the meta words; nothing is launched unless it returns RGBD_OK
int validate(const int32_t* mh, int N, int B, int H, int W, bool one_size, long long* n_chars, int* n_resized) {
  RGBD_REQUIRE(mh && N > 0 && B > 0 && H > 0 && W > 0, RGBD_E_ARG);
  RGBD_REQUIRE((long long)H * W < (1ll << 31), RGBD_E_SHAPE);
  const Meta mt = meta_of(mh, N);
  RGBD_REQUIRE(mt.offsets[0] == 0, RGBD_E_ARG);
  int nr = 0;
  for (int m = 0; m < N; ++m) {
    const int h = mt.hw[2 * m], w = mt.hw[2 * m + 1];
    RGBD_REQUIRE(mt.offsets[m + 1] >= mt.offsets[m] && h > 0 && w > 0, RGBD_E_ARG);
    RGBD_REQUIRE((long long)h * w < (1ll << 31), RGBD_E_SHAPE);
    RGBD_REQUIRE(mt.take[m] == 0 || mt.take[m] == 1, RGBD_E_ARG);
    if (h != H || w != W) {
      RGBD_REQUIRE(!one_size, RGBD_E_ARG);
      RGBD_REQUIRE(mt.slot[m] == nr && mt.resized[nr] == m, RGBD_E_ARG);
      ++nr;
    } else {
      RGBD_REQUIRE(mt.slot[m] == -1, RGBD_E_ARG);
    }
  }
  RGBD_REQUIRE(mt.ranges[0] == 0 && mt.ranges[B] == N, RGBD_E_ARG);
  for (int b = 0; b < B; ++b) RGBD_REQUIRE(mt.ranges[b + 1] >= mt.ranges[b], RGBD_E_ARG);
  *n_chars = mt.offsets[N];
  *n_resized = nr;
  return RGBD_OK;
}

inline int paint_grid(int H, int W) { return ceil_div((long long)H * ((W + RLE_PX - 1) / RLE_PX), 256); }

}  // namespace
}  // namespace rgbd

using namespace rgbd;

extern "C" {

int rgbd_rle_chunk(void) { return RLE_CHUNK; }

size_t rgbd_rle_workspace_size(int n_masks, long long n_chars, int n_resized, int H, int W) {
  if (n_masks <= 0 || n_chars < 0 || n_resized < 0 || H <= 0 || W <= 0) return 0;
  return align256((size_t)n_chars * sizeof(uint32_t)) +
         align256((size_t)n_resized * ((size_t)H + (size_t)W) * sizeof(int));
}

int rgbd_rle_counts(const uint8_t* chars, const int32_t* meta_host, const int32_t* meta_dev, int N, int B, int H,
                    int W, uint32_t* ends, int32_t* info, void* stream) {
  RGBD_REQUIRE(chars && meta_dev && ends && info, RGBD_E_ARG);
  long long n_chars;
  int n_resized;
  const int rc = validate(meta_host, N, B, H, W, false, &n_chars, &n_resized);
  if (rc != RGBD_OK) return rc;
  hipLaunchKernelGGL(k_rle_counts, dim3(N), dim3(RLE_CHUNK), 0, (hipStream_t)stream, chars, meta_dev, N, H, W, ends,
                     info);
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

int rgbd_rle_paint(const uint8_t* chars, const int32_t* meta_host, const int32_t* meta_dev, int N, int B, int H, int W,
                   int32_t* out, int32_t* info, void* ws, void* stream) {
  RGBD_REQUIRE(chars && meta_dev && out && info && ws && ((uintptr_t)out & 15) == 0, RGBD_E_ARG);
  long long n_chars;
  int n_resized;
  const int rc = validate(meta_host, N, B, H, W, false, &n_chars, &n_resized);
  if (rc != RGBD_OK) return rc;
  RGBD_REQUIRE(B <= 65535 && n_resized <= 65535, RGBD_E_SHAPE);
  hipStream_t s = (hipStream_t)stream;
  uint32_t* ends = (uint32_t*)ws;
  int* tabs = (int*)((char*)ws + align256((size_t)n_chars * sizeof(uint32_t)));
  hipLaunchKernelGGL(k_rle_counts, dim3(N), dim3(RLE_CHUNK), 0, s, chars, meta_dev, N, H, W, ends, info);
  RGBD_CHECK_LAUNCH();
  if (n_resized > 0) {
    hipLaunchKernelGGL(k_rle_tables, dim3(n_resized), dim3(64), 0, s, meta_dev, N, H, W, tabs);
    RGBD_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_rle_any_set, dim3(ceil_div((long long)H * W, 256), n_resized), dim3(256), 0, s, meta_dev, N,
                       H, W, ends, tabs, info);
    RGBD_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_rle_paint<false>, dim3(paint_grid(H, W), B), dim3(256), 0, s, meta_dev, N, H, W, ends, tabs,
                     info, (void*)out);
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

int rgbd_rle_stack(const uint8_t* chars, const int32_t* meta_host, const int32_t* meta_dev, int N, int h, int w,
                   uint8_t* out, int32_t* info, void* ws, void* stream) {
  RGBD_REQUIRE(chars && meta_dev && out && info && ws && ((uintptr_t)out & 3) == 0, RGBD_E_ARG);
  long long n_chars;
  int n_resized;
  const int rc = validate(meta_host, N, 1, h, w, true, &n_chars, &n_resized);
  if (rc != RGBD_OK) return rc;
  RGBD_REQUIRE(N <= 65535, RGBD_E_SHAPE);
  hipStream_t s = (hipStream_t)stream;
  uint32_t* ends = (uint32_t*)ws;
  hipLaunchKernelGGL(k_rle_counts, dim3(N), dim3(RLE_CHUNK), 0, s, chars, meta_dev, N, h, w, ends, info);
  RGBD_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_rle_paint<true>, dim3(paint_grid(h, w), N), dim3(256), 0, s, meta_dev, N, h, w, ends,
                     (const int*)ends, info, (void*)out);
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

}  // extern "C"
