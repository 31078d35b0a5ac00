// f6: matching the segments of two label maps on the device (gfx950).
//
// Reference: mask2former/predictor.py:181-292 (_create_consistent_prediction_overlay) cuts a
// prediction map and a ground-truth map into one boolean mask per listed segment, :95-155
// (match_predictions_to_gt) takes the IoU of every pair (:72-92 calculate_mask_iou: P G full-frame
// logical_and / logical_or passes) and matches greedily by descending IoU, and :266-284 paints a
// matched segment in its GT instance's colour and every other one in the "unmatched" colour.
// The masks of one map are disjoint, so everything the reference counts is a cell, a row sum or a
// column sum of the contingency table of the two maps:
//
//   k_contingency     one pass over both maps, 8 B per pixel.  counts[b][i][j] = pixels naming id i in
//                     a and id j in b; index na (nb) is the "none" row (column): NaN, fractions,
//                     negatives and ids past the range (cell_id, label_cell.hpp).  One workgroup
//                     column per image (grid.y); a lane takes VEC consecutive cells of the flat
//                     [B H W] range: VEC = 4 with one 16-byte load per map when both maps are
//                     16-byte aligned, VEC = 1 for 4-byte-aligned views.  A group may straddle two
//                     images; each image's workgroups count only the cells inside their image.
//                     Accumulation (HIP guide, Guideline 12): label maps are piecewise constant, so
//                     per cell slot the wave first agrees on its first active lane's key — every
//                     lane holding that key is counted by one add of the popcount, the other lanes
//                     add 1 themselves.  With (na+1)(nb+1) int32 <= 160 KB the adds go to a table in
//                     LDS, which the workgroup flushes with one integer global atomic per non-zero
//                     cell; larger tables take the same adds straight to the zeroed global table.
//                     Integer adds commute, so the table is bitwise reproducible under any schedule
//                     (no entry in the deterministic-mode switch).
//   k_greedy_match    one workgroup per image.  Areas are the row and column sums (LDS atomics over
//                     the non-zero cells); listed ids with area 0 (or outside the range, the -1
//                     padding included) are dropped, as the reference drops empty masks, and every
//                     index below is a position in these filtered lists.
//                     IoU = inter / (area_a + area_b - inter) by one float64 DIVISION, 0 when the
//                     union is 0 — the reference's own expression (NumPy int64 / int64 -> float64),
//                     so the comparison with the threshold (>=) sees the reference's double.  With
//                     fewer than 2^21 pixels two distinct such rationals never round to the same
//                     double (they differ by >= 2^-42 relatively > 2^-52), so ordering by the
//                     quotient is ordering by the rational and ties are exactly the equal rationals.
//                     Matching: repeat { among the pairs (i, j) with IoU >= threshold, i unmatched,
//                     j unused, take the one of largest IoU, then smallest i, then smallest j }.
//                     This is the reference's result: its candidates are appended in (i, j)
//                     lexicographic order and sorted by IoU descending with Python's stable sort, so
//                     they stand in (IoU desc, i asc, j asc) order; its sweep accepts a candidate
//                     iff both sides are still free.  The first candidate it accepts is the first of
//                     the order.  After an acceptance every candidate sharing its i or j is refused
//                     for good, candidates before the accepted one were all accepted or refused
//                     already, so the next one it accepts is the first of the order among those
//                     whose sides are both free — the pair the loop above takes.  Induction over
//                     the acceptances gives the same matching.
//                     Thread i keeps row i's best free candidate; a round is one workgroup
//                     reduction, and only the rows whose best column was just taken rescan.
//   k_match_lut       the colour table rgbd_overlay_blend takes.  Mode 0 ("gt") restates
//                     predictor.py:266-284, including its indexing: the i-th LISTED segment is
//                     coloured by entry i of the FILTERED match arrays.  Mode 1
//                     ("track"): palette[track % n_colors].
//   k_track_assign    stable ids for a stream: a matched segment inherits the previous frame's
//                     track, the other non-empty ones take fresh numbers in ascending id order.
#include <algorithm>
#include <cmath>

#include "common.hpp"
#include "label_cell.hpp"

using namespace rgbd;

namespace {

constexpr int SM_THR = 256;
constexpr int SM_MAX_IDS = 256;          // na, nb, La, Lb
constexpr int SM_LDS_BYTES = 163840;     // the workgroup's LDS on gfx950
constexpr long long SM_MAX_HW = 1ll << 21;  // match: denominators below 2^21 (see above)

__global__ __launch_bounds__(SM_THR) void k_zero_i32(int32_t* p, long long n) {
  const long long i = blockIdx.x * (long long)SM_THR + threadIdx.x;
  if (i < n) p[i] = 0;
}

// Every lane of the wave calls this; key < 0 adds nothing.
__device__ __forceinline__ void wave_add(int32_t* table, int key) {
  const unsigned long long act = __ballot(key >= 0);
  if (act == 0) return;
  const int lead = __shfl(key, __ffsll((long long)act) - 1);
  const unsigned long long same = __ballot(key == lead);
  if (key == lead) {
    if ((int)(threadIdx.x & 63) == __ffsll((long long)same) - 1) atomicAdd(&table[lead], (int32_t)__popcll(same));
  } else if (key >= 0) {
    atomicAdd(&table[key], 1);
  }
}

template <int VEC, bool AF32, bool BF32, bool LDS>
__global__ __launch_bounds__(SM_THR) void k_contingency(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                       long long npix, long long hw, int na, int nb,
                                                       int32_t* __restrict__ counts) {
  extern __shared__ int32_t sm_tab[];
  const int img = blockIdx.y;
  const int nb1 = nb + 1;
  const int T = (na + 1) * nb1;
  int32_t* out = counts + (long long)img * T;
  if constexpr (LDS) {
    for (int i = threadIdx.x; i < T; i += SM_THR) sm_tab[i] = 0;
    __syncthreads();
  }
  int32_t* acc = LDS ? sm_tab : out;
  const long long p_beg = img * hw, p_end = p_beg + hw;
  const long long g_end = (p_end + VEC - 1) / VEC;
  // the trip count is the same for every lane of the workgroup: wave_add needs whole waves
  for (long long base = p_beg / VEC + blockIdx.x * (long long)SM_THR; base < g_end;
       base += gridDim.x * (long long)SM_THR) {
    const long long p0 = (base + threadIdx.x) * VEC;
    uint32_t ca[VEC], cb[VEC];
    if (VEC == 4 && p0 + 4 <= npix) {
      const u32x4 va = *reinterpret_cast<const u32x4*>(a + p0);
      const u32x4 vb = *reinterpret_cast<const u32x4*>(b + p0);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        ca[k] = va[k];
        cb[k] = vb[k];
      }
    } else {
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const bool in = p0 + k < npix;
        ca[k] = in ? a[p0 + k] : 0u;
        cb[k] = in ? b[p0 + k] : 0u;
      }
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const long long p = p0 + k;
      int key = -1;
      if (p >= p_beg && p < p_end) {  // this image's cells only (p_end <= npix)
        const int ia = cell_id<AF32>(ca[k], na), ib = cell_id<BF32>(cb[k], nb);
        key = (ia < 0 ? na : ia) * nb1 + (ib < 0 ? nb : ib);
      }
      wave_add(acc, key);
    }
  }
  if constexpr (LDS) {
    __syncthreads();
    for (int i = threadIdx.x; i < T; i += SM_THR) {
      const int32_t v = sm_tab[i];
      if (v) atomicAdd(&out[i], v);
    }
  }
}

template <int VEC, bool AF32, bool BF32, bool LDS>
int launch_contingency(const void* a, const void* b, long long npix, long long hw, int B, int na, int nb, int32_t* counts,
                       hipStream_t s) {
  auto* kern = k_contingency<VEC, AF32, BF32, LDS>;
  const size_t table = (size_t)(na + 1) * (nb + 1) * 4;
  if constexpr (LDS) {
    static const hipError_t attr =
        hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, SM_LDS_BYTES);
    if (attr != hipSuccess) return (int)attr;
  }
  // a big LDS table costs a zeroing and a flush per workgroup and leaves one workgroup per CU:
  // about one workgroup per CU then, four times as many for small tables
  const long long groups = hw / VEC + 2;
  const long long cap = std::max<long long>(1, (table > 16384 ? 256 : 1024) / B);
  const unsigned gx = (unsigned)std::min<long long>(std::max<long long>(1, (groups + SM_THR - 1) / SM_THR), cap);
  kern<<<dim3(gx, B), SM_THR, LDS ? table : 0, s>>>((const uint32_t*)a, (const uint32_t*)b, npix, hw, na, nb, counts);
  return RGBD_OK;
}

template <int VEC, bool LDS>
int dispatch_dtypes(bool af, bool bf, const void* a, const void* b, long long npix, long long hw, int B, int na, int nb,
                    int32_t* counts, hipStream_t s) {
  if (af) return bf ? launch_contingency<VEC, true, true, LDS>(a, b, npix, hw, B, na, nb, counts, s)
                    : launch_contingency<VEC, true, false, LDS>(a, b, npix, hw, B, na, nb, counts, s);
  return bf ? launch_contingency<VEC, false, true, LDS>(a, b, npix, hw, B, na, nb, counts, s)
            : launch_contingency<VEC, false, false, LDS>(a, b, npix, hw, B, na, nb, counts, s);
}

// ---- the per-image stages: one workgroup of SM_THR threads per image

struct Areas {
  int a[SM_MAX_IDS], b[SM_MAX_IDS];
};

// row and column sums of one image's table, the "none" column / row included in the sums
__device__ void table_areas(const int32_t* __restrict__ tab, int na, int nb, Areas& ar) {
  for (int i = threadIdx.x; i < SM_MAX_IDS; i += SM_THR) ar.a[i] = ar.b[i] = 0;
  __syncthreads();
  const int nb1 = nb + 1, T = (na + 1) * nb1;
  for (int idx = threadIdx.x; idx < T; idx += SM_THR) {
    const int32_t c = tab[idx];
    if (c) {
      const int r = idx / nb1, col = idx - r * nb1;
      if (r < na) atomicAdd(&ar.a[r], c);
      if (col < nb) atomicAdd(&ar.b[col], c);
    }
  }
  __syncthreads();
}

// the listed ids that name a non-empty segment, in list order (one thread); -> their number
__device__ int filter_list(const int32_t* __restrict__ list, int L, const int* area, int n, int* kept) {
  int m = 0;
  for (int t = 0; t < L; ++t) {
    const int id = list[t];
    if (id >= 0 && id < n && area[id] > 0) kept[m++] = id;
  }
  return m;
}

__device__ __forceinline__ double pair_iou(int32_t inter, int area_a, int area_b) {
  const long long uni = (long long)area_a + area_b - inter;
  return uni > 0 ? (double)inter / (double)uni : 0.0;
}

__global__ __launch_bounds__(SM_THR) void k_greedy_match(const int32_t* __restrict__ counts, int na, int nb,
                                                        const int32_t* __restrict__ a_list, int La,
                                                        const int32_t* __restrict__ b_list, int Lb, double thr,
                                                        int32_t* __restrict__ matched, int32_t* __restrict__ b_count,
                                                        int32_t* __restrict__ n_filtered) {
  __shared__ Areas ar;
  __shared__ int fa[SM_MAX_IDS], fb[SM_MAX_IDS], best_j[SM_MAX_IDS], match_s[SM_MAX_IDS], used[SM_MAX_IDS];
  __shared__ int n_s[2];
  __shared__ unsigned long long red_k[SM_THR / 64];
  __shared__ int red_i[SM_THR / 64];
  const int img = blockIdx.x, t = threadIdx.x;
  const int nb1 = nb + 1;
  const int32_t* tab = counts + (long long)img * (na + 1) * nb1;
  table_areas(tab, na, nb, ar);
  if (t == 0) n_s[0] = filter_list(a_list + (long long)img * La, La, ar.a, na, fa);
  if (t == 64) n_s[1] = filter_list(b_list + (long long)img * Lb, Lb, ar.b, nb, fb);
  match_s[t] = -1;
  used[t] = 0;
  __syncthreads();
  const int pa = n_s[0], pb = n_s[1];

  // row t's best free candidate: key = IoU's bits + 1 (IoU in [0, 1]: the bits order as the values), 0 = none
  unsigned long long key = 0;
  bool done = t >= pa;
  auto rescan = [&]() {
    key = 0;
    int bj = -1;
    const int32_t* row = tab + fa[t] * nb1;
    const int area_a = ar.a[fa[t]];
    for (int j = 0; j < pb; ++j) {
      if (used[j]) continue;
      const double iou = pair_iou(row[fb[j]], area_a, ar.b[fb[j]]);
      if (iou >= thr) {
        const unsigned long long k = (unsigned long long)__double_as_longlong(iou) + 1ull;
        if (k > key) {  // strict: of equal IoUs the smallest j stays
          key = k;
          bj = j;
        }
      }
    }
    best_j[t] = bj;
  };
  if (!done) rescan();
  __syncthreads();
  for (;;) {
    unsigned long long k = done ? 0ull : key;
    int i = t;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long ok = __shfl_xor(k, o);
      const int oi = __shfl_xor(i, o);
      if (ok > k || (ok == k && oi < i)) {
        k = ok;
        i = oi;
      }
    }
    if ((t & 63) == 0) {
      red_k[t >> 6] = k;
      red_i[t >> 6] = i;
    }
    __syncthreads();
    k = red_k[0];
    i = red_i[0];
#pragma unroll
    for (int w = 1; w < SM_THR / 64; ++w)
      if (red_k[w] > k) {  // waves hold ascending rows: strict keeps the smallest i
        k = red_k[w];
        i = red_i[w];
      }
    if (k == 0) break;  // the same for every thread
    const int j = best_j[i];
    __syncthreads();    // everyone has read red_* and best_j[i]
    if (t == i) {
      done = true;
      match_s[i] = j;
      used[j] = 1;
    }
    __syncthreads();
    if (!done && best_j[t] == j) rescan();
  }
  if (t < La) matched[(long long)img * La + t] = t < pa ? match_s[t] : -1;
  if (t < Lb) b_count[(long long)img * Lb + t] = t < pb ? used[t] : 0;
  if (t < 2) n_filtered[2 * img + t] = n_s[t];
}

__global__ __launch_bounds__(SM_THR) void k_match_lut_gt(const int32_t* __restrict__ counts, int na, int nb,
                                                        const int32_t* __restrict__ a_list, int La,
                                                        const int32_t* __restrict__ b_list, int Lb,
                                                        const int32_t* __restrict__ matched,
                                                        const int32_t* __restrict__ n_filtered,
                                                        const int32_t* __restrict__ gt_colors, int32_t unmatched,
                                                        int32_t* __restrict__ lut) {
  __shared__ Areas ar;
  __shared__ int fb[SM_MAX_IDS];
  __shared__ int pb_s;
  const int img = blockIdx.x, t = threadIdx.x;
  table_areas(counts + (long long)img * (na + 1) * (nb + 1), na, nb, ar);
  if (t == 0) pb_s = filter_list(b_list + (long long)img * Lb, Lb, ar.b, nb, fb);
  for (int id = t; id < na; id += SM_THR) lut[(long long)img * na + id] = -1;
  __syncthreads();
  const int pa = n_filtered[2 * img];
  if (t < La) {
    const int id = a_list[(long long)img * La + t];
    if (id >= 0 && id < na && ar.a[id] > 0) {
      int32_t col = unmatched;
      // the reference indexes the filtered arrays with the position in segments_info
      const int m = t < pa ? matched[(long long)img * La + t] : -1;
      if (m >= 0 && m < pb_s) {
        const int32_t c = gt_colors[(long long)img * nb + fb[m]];
        if (c >= 0) col = c;
      }
      lut[(long long)img * na + id] = col;
    }
  }
}

__global__ __launch_bounds__(SM_THR) void k_match_lut_track(const int32_t* __restrict__ track,
                                                           const uint8_t* __restrict__ palette, int n_colors, int n_ids,
                                                           int32_t* __restrict__ lut) {
  const int id = blockIdx.x * SM_THR + threadIdx.x;
  if (id >= n_ids) return;
  const long long at = (long long)blockIdx.y * n_ids + id;
  const int32_t tr = track[at];
  int32_t v = -1;
  if (tr >= 0) {
    const uint8_t* p = palette + 3 * (tr % n_colors);
    v = (int32_t)p[0] | ((int32_t)p[1] << 8) | ((int32_t)p[2] << 16);
  }
  lut[at] = v;
}

__global__ __launch_bounds__(SM_THR) void k_track_assign(const int32_t* __restrict__ counts, int Q,
                                                        const int32_t* __restrict__ matched,
                                                        const int32_t* __restrict__ prev_track,
                                                        int32_t* __restrict__ next_track, int32_t* __restrict__ track) {
  __shared__ Areas ar;
  __shared__ int fb[SM_MAX_IDS];
  const int img = blockIdx.x;
  table_areas(counts + (long long)img * (Q + 1) * (Q + 1), Q, Q, ar);
  if (threadIdx.x != 0) return;
  // a_list = b_list = 0..Q-1: the filtered lists are the non-empty ids in ascending order
  int pb = 0;
  for (int id = 0; id < Q; ++id)
    if (ar.b[id] > 0) fb[pb++] = id;
  int next = next_track[img], pos = 0;
  for (int id = 0; id < Q; ++id) {
    int32_t tr = -1;
    if (ar.a[id] > 0) {
      const int m = matched[(long long)img * Q + pos++];
      tr = (m >= 0 && m < pb) ? prev_track[(long long)img * Q + fb[m]] : -1;
      if (tr < 0) tr = next++;
    }
    track[(long long)img * Q + id] = tr;
  }
  next_track[img] = next;
}

bool id_ranges_ok(int na, int nb) { return na <= SM_MAX_IDS && nb <= SM_MAX_IDS; }

}  // namespace

extern "C" {

int rgbd_label_contingency(const void* a, int a_dtype, const void* b, int b_dtype, int B, int H, int W, int na, int nb,
                           int32_t* counts, void* stream) {
  RGBD_REQUIRE(a && b && counts, RGBD_E_ARG);
  RGBD_REQUIRE(B > 0 && H > 0 && W > 0 && na > 0 && nb > 0, RGBD_E_ARG);
  RGBD_REQUIRE((a_dtype == RGBD_F32 || a_dtype == RGBD_I32) && (b_dtype == RGBD_F32 || b_dtype == RGBD_I32),
               RGBD_E_DTYPE);
  RGBD_REQUIRE(id_ranges_ok(na, nb), RGBD_E_SHAPE);
  const long long hw = (long long)H * W;
  RGBD_REQUIRE(B <= 65535 && hw < (1ll << 31), RGBD_E_SHAPE);  // one grid row per image, int32 counts
  RGBD_REQUIRE((((uintptr_t)a | (uintptr_t)b | (uintptr_t)counts) & 3) == 0, RGBD_E_ARG);
  hipStream_t s = (hipStream_t)stream;
  const long long npix = hw * B;
  const long long cells = (long long)B * (na + 1) * (nb + 1);
  k_zero_i32<<<(unsigned)((cells + SM_THR - 1) / SM_THR), SM_THR, 0, s>>>(counts, cells);
  const bool lds = (size_t)(na + 1) * (nb + 1) * 4 <= (size_t)SM_LDS_BYTES;
  const bool vec = (((uintptr_t)a | (uintptr_t)b) & 15) == 0;
  const bool af = a_dtype == RGBD_F32, bf = b_dtype == RGBD_F32;
  int rc;
  if (vec)
    rc = lds ? dispatch_dtypes<4, true>(af, bf, a, b, npix, hw, B, na, nb, counts, s)
             : dispatch_dtypes<4, false>(af, bf, a, b, npix, hw, B, na, nb, counts, s);
  else
    rc = lds ? dispatch_dtypes<1, true>(af, bf, a, b, npix, hw, B, na, nb, counts, s)
             : dispatch_dtypes<1, false>(af, bf, a, b, npix, hw, B, na, nb, counts, s);
  if (rc != RGBD_OK) return rc;
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

int rgbd_greedy_iou_match(const int32_t* counts, int B, int na, int nb, long long hw, const int32_t* a_list, int La,
                          const int32_t* b_list, int Lb, double iou_threshold, int32_t* matched,
                          int32_t* b_match_count, int32_t* n_filtered, void* stream) {
  RGBD_REQUIRE(counts && a_list && b_list && matched && b_match_count && n_filtered, RGBD_E_ARG);
  RGBD_REQUIRE(B > 0 && na > 0 && nb > 0 && hw > 0 && La > 0 && Lb > 0, RGBD_E_ARG);
  RGBD_REQUIRE(std::isfinite(iou_threshold), RGBD_E_ARG);
  RGBD_REQUIRE(id_ranges_ok(na, nb) && La <= SM_MAX_IDS && Lb <= SM_MAX_IDS && hw <= SM_MAX_HW, RGBD_E_SHAPE);
  k_greedy_match<<<B, SM_THR, 0, (hipStream_t)stream>>>(counts, na, nb, a_list, La, b_list, Lb, iou_threshold, matched,
                                                       b_match_count, n_filtered);
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

int rgbd_match_lut(int mode, const int32_t* counts, int B, int na, int nb, const int32_t* a_list, int La,
                   const int32_t* b_list, int Lb, const int32_t* matched, const int32_t* n_filtered,
                   const int32_t* gt_colors, int32_t unmatched_color, const int32_t* track, const uint8_t* palette,
                   int n_colors, int32_t* lut, void* stream) {
  RGBD_REQUIRE(mode == 0 || mode == 1, RGBD_E_ARG);
  RGBD_REQUIRE(lut && B > 0 && na > 0, RGBD_E_ARG);
  if (mode == 0) {
    RGBD_REQUIRE(counts && a_list && b_list && matched && n_filtered && gt_colors, RGBD_E_ARG);
    RGBD_REQUIRE(nb > 0 && La > 0 && Lb > 0 && unmatched_color >= 0 && unmatched_color < (1 << 24), RGBD_E_ARG);
    RGBD_REQUIRE(id_ranges_ok(na, nb) && La <= SM_MAX_IDS && Lb <= SM_MAX_IDS, RGBD_E_SHAPE);
    k_match_lut_gt<<<B, SM_THR, 0, (hipStream_t)stream>>>(counts, na, nb, a_list, La, b_list, Lb, matched, n_filtered,
                                                         gt_colors, unmatched_color, lut);
  } else {
    RGBD_REQUIRE(track && palette && n_colors > 0, RGBD_E_ARG);
    RGBD_REQUIRE(B <= 65535 && na <= SM_MAX_IDS, RGBD_E_SHAPE);
    k_match_lut_track<<<dim3(ceil_div(na, SM_THR), B), SM_THR, 0, (hipStream_t)stream>>>(track, palette, n_colors, na,
                                                                                        lut);
  }
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

int rgbd_track_assign(const int32_t* counts, int B, int Q, const int32_t* matched, const int32_t* prev_track,
                      int32_t* next_track, int32_t* track, void* stream) {
  RGBD_REQUIRE(counts && matched && prev_track && next_track && track, RGBD_E_ARG);
  RGBD_REQUIRE(B > 0 && Q > 0, RGBD_E_ARG);
  RGBD_REQUIRE(Q <= SM_MAX_IDS, RGBD_E_SHAPE);
  k_track_assign<<<B, SM_THR, 0, (hipStream_t)stream>>>(counts, Q, matched, prev_track, next_track, track);
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

}  // extern "C"
