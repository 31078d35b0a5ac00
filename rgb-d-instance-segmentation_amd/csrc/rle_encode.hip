// f4: compressed COCO RLE strings, boxes and areas encoded on the device — the
// writing half of the reference's per-image JSON (mask2former/predictor.py:376-457 and :528-625 over
// pycocotools.mask.encode; the C routines are maskApi.c rleEncode and rleToString, the box is
// _calculate_bbox_from_mask, predictor.py:460-490).  Integer-only; every output word and byte has
// one writer, so two runs give the same bytes.
//
// A mask is a predicate over the cells of a plane: cell == ids[m] of image m / Q's label map
// (label-map mode; the [N, h, w] stack is never formed) or cell != 0 of plane m (stack mode).
//
// k_enc_transpose  the planes once into column-major order (p = x h + y, maskApi's order), as the
//                  id each cell names (int16, -1 = none; label_cell.hpp) or as a 0 | 1 byte, through
//                  a 32 x 32 LDS tile.  Every later read of a mask is then a contiguous 8-cell vector.
// k_enc_count      grid (segments, masks): a workgroup takes RLE_ENC_STEPS steps of RLE_ENC_CHUNK
//                  cells (8 per lane) of one mask and counts the boundaries (cells whose predicate
//                  differs from the cell before), the set cells and their box -> one partial per
//                  (mask, segment).
// k_enc_scan_counts one workgroup: per mask the partials in segment order (each segment's first
//                  boundary index, the area, the box), the number of counts = boundaries + 1 (+ 1 for
//                  the leading 0 count of a mask whose cell 0 is set), and the scan over masks that
//                  places each mask's run ends in the one `ends` buffer; a mask that would pass
//                  cap_counts gets RLE_ENC_NO_COUNTS.
// k_enc_runs       the grid of k_enc_count again: the scan of the boundary flags numbers them, and
//                  boundary k at cell p is the end of run k: E[k] = p; the last run ends at h w.
//                  Counts are E's differences, which is all the string stage reads.
// k_enc_string<false>  one workgroup per mask, 256 counts per step: x[i] = cnt[i] - cnt[i-2] (i > 2),
//                  its 5-bit groups -> the mask's number of characters.
// k_enc_scan_chars one workgroup: the scan over masks -> offsets [N+1]; a mask that would pass
//                  cap_chars gets RLE_ENC_NO_CHARS and no characters.
// k_enc_string<true>   the same walk; the scan of the lengths places each count's characters.
// Bound: the N passes over the transposed plane in k_enc_count / k_enc_runs (2 bytes per cell and
//   mask, contiguous), not the string stage.
#include <type_traits>

#include "common.hpp"
#include "label_cell.hpp"

namespace rgbd {
namespace {

constexpr int RLE_ENC_LANE = 8;                       // cells per lane and step
constexpr int RLE_ENC_CHUNK = 256 * RLE_ENC_LANE;     // cells per workgroup step
constexpr int RLE_ENC_STEPS = 4;                      // steps per workgroup
constexpr long long RLE_ENC_SEG = (long long)RLE_ENC_CHUNK * RLE_ENC_STEPS;  // cells per segment
constexpr int RLE_ENC_PART = 6;                       // words per partial: boundaries, area, x0, y0, x1, y1
constexpr int RLE_ENC_NO_COUNTS = 1;                  // the mask's counts passed cap_counts
constexpr int RLE_ENC_NO_CHARS = 2;                   // the mask's characters passed cap_chars
constexpr int RLE_ENC_MAX_MASKS = 65535;
constexpr int MODE_LABELS = 0, MODE_STACK = 1;

typedef unsigned long long u64;

inline long long plane_stride(long long L) { return (L + RLE_ENC_LANE - 1) / RLE_ENC_LANE * RLE_ENC_LANE; }
inline int n_segments(long long L) { return (int)((L + RLE_ENC_SEG - 1) / RLE_ENC_SEG); }

// workspace: planes | partials int32 [N][S][6] | coff u64 [N+1] | len u64 [N] | ends uint32 [cap_counts]
struct Ws {
  char* planes;
  int32_t* part;
  u64 *coff, *len;
  uint32_t* ends;
  size_t bytes;
};
inline Ws ws_of(void* base, int mode, int n_images, int n_masks, long long L, long long cap_counts) {
  Ws w;
  char* p = (char*)base;
  const size_t planes = mode == MODE_STACK ? (size_t)n_masks : (size_t)n_images;
  w.planes = p;
  p += align256(planes * (size_t)plane_stride(L) * (mode == MODE_STACK ? 1 : 2));
  w.part = (int32_t*)p;
  p += align256((size_t)n_masks * n_segments(L) * RLE_ENC_PART * sizeof(int32_t));
  w.coff = (u64*)p;
  p += align256(((size_t)n_masks + 1) * sizeof(u64));
  w.len = (u64*)p;
  p += align256((size_t)n_masks * sizeof(u64));
  w.ends = (uint32_t*)p;
  p += align256((size_t)cap_counts * sizeof(uint32_t));
  w.bytes = (size_t)(p - (char*)base);
  return w;
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
  for (int k = 0; k < 4; ++k) {
    const T s = sh[k];
    if (k < wv) add += s;
    tot += s;
  }
  __syncthreads();
  total = tot;
  return v + add;
}

// SRC 0: float32 label map, 1: int32 label map (-> int16 ids), 2: uint8 stack (-> 0 | 1 bytes)
template <int SRC>
__global__ __launch_bounds__(256) void k_enc_transpose(const void* __restrict__ src, int H, int W, int n_ids,
                                                        long long stride, void* __restrict__ dst) {
  typedef typename std::conditional<SRC == 2, uint8_t, int16_t>::type C;
  __shared__ C tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int x0 = blockIdx.x * 32, y0 = blockIdx.y * 32;
  const size_t plane = blockIdx.z;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int y = y0 + ty + 8 * k, x = x0 + tx;
    C c = 0;
    if (y < H && x < W) {
      const size_t at = (plane * H + y) * W + x;
      if constexpr (SRC == 2)
        c = ((const uint8_t*)src)[at] != 0 ? 1 : 0;
      else
        c = (C)cell_id<SRC == 0>(((const uint32_t*)src)[at], n_ids);
    }
    tile[ty + 8 * k][tx] = c;
  }
  __syncthreads();
  C* out = (C*)dst + plane * (size_t)stride;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = x0 + ty + 8 * k, y = y0 + tx;
    if (x < W && y < H) out[(size_t)x * H + y] = tile[tx][ty + 8 * k];
  }
}

// The predicate bits of the 8 cells from p0 (bit q = cell p0 + q; cells at or past L read as 0) of
// a column-major plane.  p0 is a multiple of 8 below the plane's stride, so the vector is aligned
// and inside the plane's slot.
template <bool STACK>
__device__ __forceinline__ unsigned cell_bits(const void* plane, uint32_t p0, uint32_t L, int id) {
  unsigned bits = 0;
  if constexpr (STACK) {
    const uint2 v = *(const uint2*)((const uint8_t*)plane + p0);
    const uint32_t w[2] = {v.x, v.y};
#pragma unroll
    for (int q = 0; q < 8; ++q) bits |= ((w[q >> 2] >> (8 * (q & 3))) & 0xffu) ? 1u << q : 0u;
  } else {
    const uint4 v = *(const uint4*)((const int16_t*)plane + p0);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 8; ++q) bits |= ((int)(int16_t)(w[q >> 1] >> (16 * (q & 1))) == id) ? 1u << q : 0u;
  }
  const uint32_t left = L - p0;  // > 0
  return left >= 8 ? bits : bits & ((1u << left) - 1u);
}
template <bool STACK>
__device__ __forceinline__ unsigned cell_bit(const void* plane, uint32_t p, int id) {
  if constexpr (STACK)
    return ((const uint8_t*)plane)[p] != 0;
  else
    return (int)((const int16_t*)plane)[p] == id;
}

// the plane and id of mask m; id < 0 (label-map mode only): an unused slot
template <bool STACK>
__device__ __forceinline__ const void* plane_of(const void* planes, long long stride, const int32_t* ids, int Q, int m,
                                                int& id) {
  if constexpr (STACK) {
    id = 0;
    return (const uint8_t*)planes + (size_t)m * stride;
  } else {
    id = ids[m];
    return (const int16_t*)planes + (size_t)(m / Q) * stride;
  }
}

// One step of a lane: the boundary flags of its 8 cells (bit q: cell p0 + q differs from the cell
// before it; cell 0 has none) and their predicate bits; 0 / 0 for a lane at or past L.
template <bool STACK>
__device__ __forceinline__ unsigned step_flags(const void* plane, uint32_t p0, uint32_t L, int id, unsigned& bits) {
  bits = 0;
  if (p0 >= L) return 0;
  bits = cell_bits<STACK>(plane, p0, L, id);
  const unsigned prev = p0 > 0 ? cell_bit<STACK>(plane, p0 - 1, id) : 0u;
  const uint32_t left = L - p0;
  const unsigned valid = left >= 8 ? 0xffu : (1u << left) - 1u;
  unsigned diff = (bits ^ ((bits << 1) | prev)) & valid;
  if (p0 == 0) diff &= ~1u;
  return diff;
}

template <bool STACK>
__global__ __launch_bounds__(256) void k_enc_count(const void* __restrict__ planes, long long stride,
                                                    const int32_t* __restrict__ ids, int Q, int H, int W,
                                                    int32_t* __restrict__ part) {
  __shared__ int sh[4][RLE_ENC_PART];
  const int m = blockIdx.y, seg = blockIdx.x, tid = threadIdx.x;
  int id;
  const void* plane = plane_of<STACK>(planes, stride, ids, Q, m, id);
  if (id < 0) return;  // block-uniform; k_enc_scan_counts does not read an unused slot's partials
  const uint32_t L = (uint32_t)H * (uint32_t)W;
  int nb = 0, area = 0, x0 = W, y0 = H, x1 = -1, y1 = -1;
  for (int st = 0; st < RLE_ENC_STEPS; ++st) {
    const long long p64 = (long long)seg * RLE_ENC_SEG + (long long)st * RLE_ENC_CHUNK + tid * RLE_ENC_LANE;
    if (p64 >= (long long)L) break;
    const uint32_t p0 = (uint32_t)p64;
    unsigned bits;
    nb += __popc(step_flags<STACK>(plane, p0, L, id, bits));
    if (bits) {
      area += __popc(bits);
      int x = (int)(p0 / (uint32_t)H), y = (int)(p0 % (uint32_t)H);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        if (bits >> q & 1) {
          x0 = min(x0, x);
          x1 = max(x1, x);
          y0 = min(y0, y);
          y1 = max(y1, y);
        }
        if (++y == H) {
          y = 0;
          ++x;
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    nb += __shfl_xor(nb, o);
    area += __shfl_xor(area, o);
    x0 = min(x0, __shfl_xor(x0, o));
    y0 = min(y0, __shfl_xor(y0, o));
    x1 = max(x1, __shfl_xor(x1, o));
    y1 = max(y1, __shfl_xor(y1, o));
  }
  if ((tid & 63) == 0) {
    int* s = sh[tid >> 6];
    s[0] = nb, s[1] = area, s[2] = x0, s[3] = y0, s[4] = x1, s[5] = y1;
  }
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < 4; ++k) {
      nb += sh[k][0];
      area += sh[k][1];
      x0 = min(x0, sh[k][2]);
      y0 = min(y0, sh[k][3]);
      x1 = max(x1, sh[k][4]);
      y1 = max(y1, sh[k][5]);
    }
    int32_t* o = part + ((size_t)m * gridDim.x + seg) * RLE_ENC_PART;
    o[0] = nb, o[1] = area, o[2] = x0, o[3] = y0, o[4] = x1, o[5] = y1;
  }
}

// one workgroup; a lane per mask.  part[m][s][0] becomes the index of segment s's first boundary.
template <bool STACK>
__global__ __launch_bounds__(256) void k_enc_scan_counts(const void* __restrict__ planes, long long stride,
                                                          const int32_t* __restrict__ ids, int Q, int N, int S, int H,
                                                          int W, long long cap_counts, int32_t* __restrict__ part,
                                                          u64* __restrict__ coff, int32_t* __restrict__ info,
                                                          long long* __restrict__ totals) {
  __shared__ u64 sh[4];
  const int tid = threadIdx.x;
  u64 carry = 0;
  if (tid == 0) coff[0] = 0;
  for (int base = 0; base < N; base += 256) {
    const int m = base + tid;
    u64 n = 0;
    int area = 0, x0 = W, y0 = H, x1 = -1, y1 = -1;
    if (m < N) {
      int id;
      const void* plane = plane_of<STACK>(planes, stride, ids, Q, m, id);
      if (id >= 0) {
        int32_t* p = part + (size_t)m * S * RLE_ENC_PART;
        uint32_t nb = 0;
        for (int s = 0; s < S; ++s, p += RLE_ENC_PART) {
          const uint32_t c = (uint32_t)p[0];
          p[0] = (int32_t)nb;
          nb += c;
          area += p[1];
          x0 = min(x0, p[2]);
          y0 = min(y0, p[3]);
          x1 = max(x1, p[4]);
          y1 = max(y1, p[5]);
        }
        n = (u64)nb + 1 + cell_bit<STACK>(plane, 0, id);
      }
    }
    u64 total;
    const u64 end = carry + block_scan<u64>(n, sh, total);
    carry += total;
    if (m < N) {
      coff[m + 1] = end;
      int32_t* o = info + 8 * (size_t)m;
      o[0] = n > 0x7fffffffull ? 0x7fffffff : (int32_t)n;
      o[1] = 0;
      o[2] = area;
      o[3] = area ? x0 : 0;
      o[4] = area ? y0 : 0;
      o[5] = area ? x1 : -1;
      o[6] = area ? y1 : -1;
      o[7] = end > (u64)cap_counts ? RLE_ENC_NO_COUNTS : 0;
    }
  }
  if (tid == 0) totals[0] = (long long)carry;
}

template <bool STACK>
__global__ __launch_bounds__(256) void k_enc_runs(const void* __restrict__ planes, long long stride,
                                                   const int32_t* __restrict__ ids, int Q, int H, int W,
                                                   const int32_t* __restrict__ part, const u64* __restrict__ coff,
                                                   const int32_t* __restrict__ info, uint32_t* __restrict__ ends) {
  __shared__ int sh[4];
  const int m = blockIdx.y, seg = blockIdx.x, tid = threadIdx.x;
  int id;
  const void* plane = plane_of<STACK>(planes, stride, ids, Q, m, id);
  if (id < 0 || info[8 * (size_t)m + 7] != 0) return;  // block-uniform: unused, or its counts do not fit
  const uint32_t L = (uint32_t)H * (uint32_t)W;
  const u64 first = cell_bit<STACK>(plane, 0, id);
  uint32_t* E = ends + coff[m];  // coff[m + 1] <= cap_counts: every index below is inside the buffer
  const u64 n = coff[m + 1] - coff[m];
  if (seg == 0 && tid == 0 && first) E[0] = 0;
  if (seg == (int)gridDim.x - 1 && tid == 0) E[n - 1] = L;
  u64 k0 = first + (u64)(uint32_t)part[((size_t)m * gridDim.x + seg) * RLE_ENC_PART];
  for (int st = 0; st < RLE_ENC_STEPS; ++st) {
    const long long c64 = (long long)seg * RLE_ENC_SEG + (long long)st * RLE_ENC_CHUNK;
    if (c64 >= (long long)L) break;  // block-uniform
    const long long p64 = c64 + tid * RLE_ENC_LANE;
    const uint32_t p0 = (uint32_t)p64;
    unsigned bits, diff = p64 < (long long)L ? step_flags<STACK>(plane, p0, L, id, bits) : 0u;
    int total;
    const int incl = block_scan<int>(__popc(diff), sh, total);
    u64 k = k0 + (u64)(incl - __popc(diff));
    while (diff) {
      const int q = __ffs(diff) - 1;
      diff &= diff - 1;
      E[k++] = p0 + q;  // k < n - 1: boundary k ends run k + first, and the last run ends at L
    }
    k0 += (u64)total;
  }
}

// the characters of count i of a mask with run ends E (maskApi.c rleToString) -> their number
__device__ __forceinline__ int count_chars(const uint32_t* E, u64 i, uint8_t* g) {
  const long long e0 = E[i], e1 = i >= 1 ? E[i - 1] : 0, e2 = i >= 2 ? E[i - 2] : 0, e3 = i >= 3 ? E[i - 3] : 0;
  long long x = e0 - e1;
  if (i > 2) x -= e2 - e3;
  int len = 0;
  bool more = true;
  while (more && len < 8) {  // |x| < 2^31: at most 7 groups
    int c = (int)(x & 0x1f);
    x >>= 5;
    more = (c & 0x10) ? x != -1 : x != 0;
    if (more) c |= 0x20;
    g[len++] = (uint8_t)(c + 48);
  }
  return len;
}

template <bool WRITE>
__global__ __launch_bounds__(256) void k_enc_string(const uint32_t* __restrict__ ends, const u64* __restrict__ coff,
                                                     const int32_t* __restrict__ info,
                                                     const int32_t* __restrict__ offsets, u64* __restrict__ len,
                                                     uint8_t* __restrict__ chars) {
  __shared__ u64 sh[4];
  const int m = blockIdx.x, tid = threadIdx.x;
  const int status = info[8 * (size_t)m + 7];
  if (WRITE ? status != 0 : (status & RLE_ENC_NO_COUNTS) != 0) {  // block-uniform
    if (!WRITE && tid == 0) len[m] = 0;
    return;
  }
  const uint32_t* E = ends + coff[m];
  const u64 n = coff[m + 1] - coff[m];
  uint8_t* out = WRITE ? chars + offsets[m] : nullptr;  // offsets[m + 1] <= cap_chars for a mask with status 0
  u64 carry = 0;
  for (u64 base = 0; base < n; base += 256) {
    const u64 i = base + tid;
    uint8_t g[8];
    const int l = i < n ? count_chars(E, i, g) : 0;
    u64 total;
    const u64 end = carry + block_scan<u64>((u64)l, sh, total);
    if (WRITE)
      for (int q = 0; q < l; ++q) out[end - l + q] = g[q];
    carry += total;
  }
  if (!WRITE && tid == 0) len[m] = carry;
}

// one workgroup; a lane per mask
__global__ __launch_bounds__(256) void k_enc_scan_chars(int N, long long cap_chars, const u64* __restrict__ len,
                                                         int32_t* __restrict__ info, int32_t* __restrict__ offsets,
                                                         long long* __restrict__ totals) {
  __shared__ u64 sh[4];
  const int tid = threadIdx.x;
  u64 need = 0, wrote = 0;
  if (tid == 0) offsets[0] = 0;
  for (int base = 0; base < N; base += 256) {
    const int m = base + tid;
    const u64 l = m < N ? len[m] : 0;
    int status = m < N ? info[8 * (size_t)m + 7] : 0;
    u64 total;
    const u64 end = need + block_scan<u64>(l, sh, total);
    need += total;
    const bool fit = status == 0 && end <= (u64)cap_chars;
    if (m < N && status == 0 && !fit) status = RLE_ENC_NO_CHARS;
    const u64 wend = wrote + block_scan<u64>(fit ? l : 0, sh, total);
    wrote += total;
    if (m < N) {
      offsets[m + 1] = (int32_t)wend;  // <= cap_chars <= 2^31 - 1
      info[8 * (size_t)m + 1] = l > 0x7fffffffull ? 0x7fffffff : (int32_t)l;
      info[8 * (size_t)m + 7] = status;
    }
  }
  if (tid == 0) totals[1] = (long long)need;
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

int check_sizes(int n_masks, int H, int W, long long cap_counts, long long cap_chars) {
  RGBD_REQUIRE(n_masks > 0 && H > 0 && W > 0 && cap_counts >= 0 && cap_chars >= 0, RGBD_E_ARG);
  RGBD_REQUIRE((long long)H * W < (1ll << 31) && n_masks <= RLE_ENC_MAX_MASKS, RGBD_E_SHAPE);
  return RGBD_OK;
}

// characters a count of a plane of L cells can take: the groups of a delta in [-L, L]
inline int max_count_chars(long long L) {
  int g = 1;
  while (g < 7 && (1ll << (5 * g - 1)) <= L) ++g;
  return g;
}

template <bool STACK>
int launch_stages(const Ws& w, int n_masks, const int32_t* ids, int Q, int H, int W, long long cap_counts,
                  long long cap_chars, uint8_t* chars, int32_t* offsets, int32_t* info, long long* totals,
                  hipStream_t s) {
  const long long L = (long long)H * W, stride = plane_stride(L);
  const int S = n_segments(L);
  if (cap_chars > 0x7fffffffll) cap_chars = 0x7fffffffll;  // offsets are int32
  const dim3 grid(S, n_masks);
  hipLaunchKernelGGL(k_enc_count<STACK>, grid, dim3(256), 0, s, (const void*)w.planes, stride, ids, Q, H, W, w.part);
  RGBD_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_enc_scan_counts<STACK>, dim3(1), dim3(256), 0, s, (const void*)w.planes, stride, ids, Q, n_masks,
                     S, H, W, cap_counts, w.part, w.coff, info, totals);
  RGBD_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_enc_runs<STACK>, grid, dim3(256), 0, s, (const void*)w.planes, stride, ids, Q, H, W,
                     (const int32_t*)w.part, (const u64*)w.coff, (const int32_t*)info, w.ends);
  RGBD_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_enc_string<false>, dim3(n_masks), dim3(256), 0, s, (const uint32_t*)w.ends, (const u64*)w.coff,
                     (const int32_t*)info, (const int32_t*)offsets, w.len, chars);
  RGBD_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_enc_scan_chars, dim3(1), dim3(256), 0, s, n_masks, cap_chars, (const u64*)w.len, info, offsets,
                     totals);
  RGBD_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_enc_string<true>, dim3(n_masks), dim3(256), 0, s, (const uint32_t*)w.ends, (const u64*)w.coff,
                     (const int32_t*)info, (const int32_t*)offsets, w.len, chars);
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

}  // namespace
}  // namespace rgbd

using namespace rgbd;

extern "C" {

int rgbd_rle_encode_chunk(void) { return RLE_ENC_CHUNK; }

int rgbd_rle_encode_capacity(int mode, int n_images, int n_masks, int H, int W, long long* counts, long long* chars) {
  RGBD_REQUIRE(counts && chars, RGBD_E_ARG);
  *counts = *chars = 0;
  RGBD_REQUIRE(mode == MODE_LABELS || mode == MODE_STACK, RGBD_E_ARG);
  if (n_images <= 0 || n_masks <= 0 || H <= 0 || W <= 0) return RGBD_OK;
  const long long L = (long long)H * W;
  // stack: a mask has at most L + 1 counts.  labels (distinct ids per image): an adjacent pair of
  // cells closes at most one run and opens at most one, 2 (L - 1) boundaries over all ids of an
  // image, and a mask has boundaries + 1 counts, + 1 for a leading 0 count.
  const long long c = mode == MODE_STACK ? (long long)n_masks * (L + 1) : (long long)n_images * 2 * (L - 1) + 2ll * n_masks;
  *counts = c;
  *chars = c * max_count_chars(L);
  return RGBD_OK;
}

size_t rgbd_rle_encode_workspace_size(int mode, int n_images, int n_masks, int H, int W, long long cap_counts) {
  if ((mode != MODE_LABELS && mode != MODE_STACK) || n_images <= 0 || n_masks <= 0 || H <= 0 || W <= 0 ||
      cap_counts < 0)
    return 0;
  return ws_of(nullptr, mode, n_images, n_masks, (long long)H * W, cap_counts).bytes;
}

int rgbd_rle_encode_labels(int dtype, const void* maps, int B, int H, int W, int n_ids, const int32_t* ids, int Q,
                           long long cap_counts, long long cap_chars, uint8_t* chars, int32_t* offsets, int32_t* info,
                           long long* totals, void* ws, void* stream) {
  RGBD_REQUIRE(maps && ids && chars && offsets && info && totals && ws, RGBD_E_ARG);
  RGBD_REQUIRE(aligned(maps, 4) && aligned(ids, 4) && aligned(offsets, 4) && aligned(info, 4) && aligned(totals, 8) &&
                   aligned(ws, 16),
               RGBD_E_ARG);
  RGBD_REQUIRE(B > 0 && Q > 0, RGBD_E_ARG);
  RGBD_REQUIRE((long long)B * Q <= RLE_ENC_MAX_MASKS, RGBD_E_SHAPE);
  const int rc = check_sizes(B * Q, H, W, cap_counts, cap_chars);
  if (rc != RGBD_OK) return rc;
  RGBD_REQUIRE(n_ids >= 1 && n_ids <= 256, RGBD_E_ARG);
  RGBD_REQUIRE(dtype == RGBD_F32 || dtype == RGBD_I32, RGBD_E_DTYPE);
  hipStream_t s = (hipStream_t)stream;
  const long long L = (long long)H * W;
  const Ws w = ws_of(ws, MODE_LABELS, B, B * Q, L, cap_counts);
  const dim3 tg(ceil_div(W, 32), ceil_div(H, 32), B);
  if (dtype == RGBD_F32)
    hipLaunchKernelGGL(k_enc_transpose<0>, tg, dim3(256), 0, s, maps, H, W, n_ids, plane_stride(L), (void*)w.planes);
  else
    hipLaunchKernelGGL(k_enc_transpose<1>, tg, dim3(256), 0, s, maps, H, W, n_ids, plane_stride(L), (void*)w.planes);
  RGBD_CHECK_LAUNCH();
  return launch_stages<false>(w, B * Q, ids, Q, H, W, cap_counts, cap_chars, chars, offsets, info, totals, s);
}

int rgbd_rle_encode_stack(const uint8_t* masks, int N, int h, int w, long long cap_counts, long long cap_chars,
                          uint8_t* chars, int32_t* offsets, int32_t* info, long long* totals, void* ws, void* stream) {
  RGBD_REQUIRE(masks && chars && offsets && info && totals && ws, RGBD_E_ARG);
  RGBD_REQUIRE(aligned(offsets, 4) && aligned(info, 4) && aligned(totals, 8) && aligned(ws, 16), RGBD_E_ARG);
  const int rc = check_sizes(N, h, w, cap_counts, cap_chars);
  if (rc != RGBD_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  const long long L = (long long)h * w;
  const Ws wk = ws_of(ws, MODE_STACK, N, N, L, cap_counts);
  hipLaunchKernelGGL(k_enc_transpose<2>, dim3(ceil_div(w, 32), ceil_div(h, 32), N), dim3(256), 0, s,
                     (const void*)masks, h, w, 1, plane_stride(L), (void*)wk.planes);
  RGBD_CHECK_LAUNCH();
  return launch_stages<true>(wk, N, nullptr, 1, h, w, cap_counts, cap_chars, chars, offsets, info, totals, s);
}

}  // extern "C"
