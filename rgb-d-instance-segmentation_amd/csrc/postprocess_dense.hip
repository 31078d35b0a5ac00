// f4b: Mask2FormerImageProcessor.post_process_semantic_segmentation and
// post_process_panoptic_segmentation on the device (transformers 5.15
// image_processing_pil_mask2former.py:587-663 and :788-881 with compute_segments :162,
// check_segment_validity :143 and remove_low_and_no_objects :245; the torchvision variant has the
// same arithmetic).  Both resize the mask logits [Q][h][w] to the fixed 384 x 384 first (bilinear,
// align_corners=False: lin_index of pp_common.hpp) and take the sigmoid after the resize.
//
// Semantic, per image:  S[c][p] = sum_q softmax(class logits)[q][c] * sigmoid(M384[q][p]), c < C
//   k_ppd_softmax     class probabilities [B][Q][C] (the no-object column dropped after the softmax)
//   k_sem_scores      one workgroup per 128-pixel tile of the 384 x 384 grid: 32 queries at a time
//                     are interpolated and squashed into LDS and contracted with their class rows
//                     (float32 fma, q ascending: a fixed order, no atomics); only S reaches memory,
//                     the [Q][384^2] probabilities never do
//   k_sem_argmax      per target pixel: four taps of S per class, running (max, index) with the
//                     first maximum winning, int64 map; the resized scores only when asked for
//
// Panoptic, per image:
//   k_pan_select      score, label = softmax.max(-1) (first maximum), kept = label != C and
//                     score > threshold, compacted in query order (one workgroup per image)
//   k_pan_argmax      per target pixel: P[k] = bilinear(sigmoid(M384[kept k])) * score[k] (the
//                     reference weighs in place, so the mask threshold below sees the weighted P),
//                     labels_px = first argmax_k, area[k] = #(labels_px == k),
//                     orig[k] = #(P[k] >= mask_threshold): integer atomics, exact in any order
//   k_pan_assign      one lane per image: valid = area > 0, orig > 0 and float32(area) /
//                     float32(orig) > overlap threshold (compared as a double, like .item());
//                     id = the id remembered for a fused label, else the running id + 1 -- the
//                     running id is *overwritten* by a remembered one, as in compute_segments
//   k_pan_paint       labels_px -> ids in place (0 where the query is not valid); an image with
//                     nothing kept gets the reference's float32 -1 map instead (same 4-byte cells)
#include "pp_common.hpp"

using namespace rgbd;

namespace {

constexpr int PP_NP = PP_S * PP_S;
constexpr int PPD_MAX_C = 1024;  // classes: the fuse set is a 1024-bit mask passed by value
constexpr int PPD_MAX_Q = 1024;  // queries: the per-image tables of the panoptic kernels live in LDS

constexpr int SEM_TP = 128;  // pixels per workgroup (two per lane)
constexpr int SEM_QC = 32;   // queries interpolated into LDS at a time
constexpr int SEM_CB = 12;   // classes per wave and pass (four waves: 48 per pass)
static_assert(PP_NP % SEM_TP == 0 && PP_S % SEM_TP == 0, "a tile is part of one row of the 384 grid");

__device__ __forceinline__ bool nan_first_gt(float v, float best) { return v > best || (v != v && best == best); }

__device__ __forceinline__ float sigmoid_at(const float* __restrict__ m, int w, const Lin& ly, const Lin& lx) {
  const float* r0 = m + (long long)ly.i0 * w;
  const float* r1 = m + (long long)ly.i1 * w;
  const float t0 = r0[lx.i0] * lx.l0 + r0[lx.i1] * lx.l1;
  const float t1 = r1[lx.i0] * lx.l0 + r1[lx.i1] * lx.l1;
  return 1.f / (1.f + expf(-(t0 * ly.l0 + t1 * ly.l1)));
}

// softmax row maximum, NaN-propagating like ATen's
__device__ __forceinline__ float row_max(const float* row, int C1) {
  float m = row[0];
  for (int c = 1; c < C1; ++c) {
    const float x = row[c];
    m = (x != x || m != m) ? __int_as_float(0x7fc00000) : fmaxf(m, x);
  }
  return m;
}

// probs [B*Q][C] = softmax(class logits [B*Q][C1])[:, :C]; one thread per row
__global__ __launch_bounds__(256) void k_ppd_softmax(const float* __restrict__ cls, int rows, int C1,
                                                     float* __restrict__ probs) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const float* row = cls + (long long)r * C1;
  const float m = row_max(row, C1);
  float s = 0.f;
  for (int c = 0; c < C1; ++c) s += expf(row[c] - m);
  for (int c = 0; c < C1 - 1; ++c) probs[(long long)r * (C1 - 1) + c] = div_rn(expf(row[c] - m), s);
}

// One image.  grid = PP_NP / SEM_TP tiles.  Filling: thread t interpolates pixel t & 127 for every
// second query of the chunk.  Contracting: lane l owns pixels 2l, 2l + 1, wave v classes
// c0 + 12 v .. + 11; the class rows are read as broadcast float4.  More than 48 classes take
// further passes, each interpolating again.
__global__ __launch_bounds__(256) void k_sem_scores(const float* __restrict__ masks, const float* __restrict__ probs,
                                                    int Q, int C, int h, int w, float* __restrict__ S) {
  __shared__ __attribute__((aligned(16))) float Ps[SEM_QC][SEM_TP];
  __shared__ __attribute__((aligned(16))) float Ws[SEM_QC][4 * SEM_CB];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int p0 = blockIdx.x * SEM_TP;
  const int ip = tid & (SEM_TP - 1), half = tid / SEM_TP;
  const int oy = (p0 + ip) / PP_S, ox = (p0 + ip) - oy * PP_S;
  const Lin ly = lin_index(oy, h, PP_S), lx = lin_index(ox, w, PP_S);
  for (int c0 = 0; c0 < C; c0 += 4 * SEM_CB) {
    float acc[SEM_CB][2];
#pragma unroll
    for (int j = 0; j < SEM_CB; ++j) acc[j][0] = acc[j][1] = 0.f;
    for (int q0 = 0; q0 < Q; q0 += SEM_QC) {
      __syncthreads();  // the previous chunk has been read
      for (int qq = half; qq < SEM_QC; qq += 256 / SEM_TP) {
        const int q = q0 + qq;
        Ps[qq][ip] = q < Q ? sigmoid_at(masks + (long long)q * h * w, w, ly, lx) : 0.f;
      }
      for (int i = tid; i < SEM_QC * 4 * SEM_CB; i += 256) {
        const int qq = i / (4 * SEM_CB), j = i - qq * (4 * SEM_CB);
        Ws[qq][j] = (q0 + qq < Q && c0 + j < C) ? probs[(long long)(q0 + qq) * C + c0 + j] : 0.f;
      }
      __syncthreads();
      if (c0 + wv * SEM_CB < C) {  // wave-uniform
#pragma unroll 4
        for (int qq = 0; qq < SEM_QC; ++qq) {
          const float2 pv = *(const float2*)&Ps[qq][2 * lane];
#pragma unroll
          for (int j4 = 0; j4 < SEM_CB / 4; ++j4) {
            const float4 wq = *(const float4*)&Ws[qq][wv * SEM_CB + 4 * j4];
            const float wj[4] = {wq.x, wq.y, wq.z, wq.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              acc[4 * j4 + j][0] = __builtin_fmaf(wj[j], pv.x, acc[4 * j4 + j][0]);
              acc[4 * j4 + j][1] = __builtin_fmaf(wj[j], pv.y, acc[4 * j4 + j][1]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < SEM_CB; ++j) {
      const int c = c0 + wv * SEM_CB + j;
      if (c < C) *(float2*)&S[(long long)c * PP_NP + p0 + 2 * lane] = make_float2(acc[j][0], acc[j][1]);
    }
  }
}

// One image: resize S [C][384][384] to (Ht, Wt) and take the argmax over the classes in one pass.
__global__ __launch_bounds__(256) void k_sem_argmax(const float* __restrict__ S, int C, int Ht, int Wt,
                                                    long long* __restrict__ map, float* __restrict__ scores) {
  const long long np = (long long)Ht * Wt;
  for (long long p = blockIdx.x * 256ll + threadIdx.x; p < np; p += 256ll * gridDim.x) {
    const int ty = (int)(p / Wt), tx = (int)(p - (long long)ty * Wt);
    const Lin ly = lin_index(ty, PP_S, Ht), lx = lin_index(tx, PP_S, Wt);
    const int o00 = ly.i0 * PP_S + lx.i0, o01 = ly.i0 * PP_S + lx.i1;
    const int o10 = ly.i1 * PP_S + lx.i0, o11 = ly.i1 * PP_S + lx.i1;
    float best = 0.f;
    int arg = 0;
    for (int c = 0; c < C; ++c) {
      const float* s = S + (long long)c * PP_NP;
      const float t0 = s[o00] * lx.l0 + s[o01] * lx.l1;
      const float t1 = s[o10] * lx.l0 + s[o11] * lx.l1;
      const float v = t0 * ly.l0 + t1 * ly.l1;
      if (scores) scores[(long long)c * np + p] = v;
      if (c == 0 || nan_first_gt(v, best)) {
        best = v;
        arg = c;
      }
    }
    map[p] = arg;
  }
}

// The per-image segment table, int32 [1 + 5 Q]: the number of kept queries, then per kept query
// (in query order) its segment id (0 = not valid), label, score (float32 bits), area and orig.
struct PanRow {
  int *nk, *id, *label, *score, *area, *orig;
};
__device__ __forceinline__ PanRow pan_row(int* table, int b, int Q) {
  int* r = table + (long long)b * (1 + 5 * Q);
  return PanRow{r, r + 1, r + 1 + Q, r + 1 + 2 * Q, r + 1 + 3 * Q, r + 1 + 4 * Q};
}

// One workgroup per image: thread per query, then lane 0 compacts in query order.
__global__ __launch_bounds__(256) void k_pan_select(const float* __restrict__ cls, int Q, int C1, float threshold,
                                                    int* __restrict__ table, int* __restrict__ keptq) {
  __shared__ float sc[PPD_MAX_Q];
  __shared__ int lb[PPD_MAX_Q];
  const int b = blockIdx.x;
  const PanRow T = pan_row(table, b, Q);
  for (int q = threadIdx.x; q < Q; q += 256) {
    const float* row = cls + ((long long)b * Q + q) * C1;
    const float m = row_max(row, C1);
    float s = 0.f;
    for (int c = 0; c < C1; ++c) s += expf(row[c] - m);
    float bp = 0.f;
    int bl = 0;
    for (int c = 0; c < C1; ++c) {
      const float p = div_rn(expf(row[c] - m), s);
      if (c == 0 || nan_first_gt(p, bp)) {
        bp = p;
        bl = c;
      }
    }
    sc[q] = bp;
    lb[q] = bl;
    T.id[q] = 0;
    T.label[q] = 0;
    T.score[q] = 0;
    T.area[q] = 0;
    T.orig[q] = 0;
    keptq[(long long)b * Q + q] = -1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int n = 0;
    for (int q = 0; q < Q; ++q)
      if (lb[q] != C1 - 1 && sc[q] > threshold) {
        keptq[(long long)b * Q + n] = q;
        T.label[n] = lb[q];
        T.score[n] = __float_as_int(sc[q]);
        ++n;
      }
    *T.nk = n;
  }
}

// Image b.  Every target pixel: the weighted probability of each kept query, the first maximum,
// and the two counts (workgroup totals in LDS, then one integer atomic per query and workgroup).
__global__ __launch_bounds__(256) void k_pan_argmax(const float* __restrict__ masks, int Q, int h, int w,
                                                    const int* __restrict__ keptq, int* __restrict__ table, int b,
                                                    int Ht, int Wt, float mask_threshold, int* __restrict__ seg) {
  __shared__ int kq[PPD_MAX_Q], ar[PPD_MAX_Q], og[PPD_MAX_Q];
  __shared__ float ks[PPD_MAX_Q];
  const PanRow T = pan_row(table, b, Q);
  const int nk = *T.nk;
  if (nk == 0) return;  // grid-uniform: k_pan_paint writes the -1 map
  for (int k = threadIdx.x; k < nk; k += 256) {
    kq[k] = keptq[(long long)b * Q + k];
    ks[k] = __int_as_float(T.score[k]);
    ar[k] = og[k] = 0;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const bool ident = Ht == PP_S && Wt == PP_S;  // no resize: one tap
  const long long np = (long long)Ht * Wt;
  for (long long base = blockIdx.x * 256ll; base < np; base += 256ll * gridDim.x) {
    const long long p = base + threadIdx.x;
    const bool valid = p < np;
    const long long pc = valid ? p : 0;
    const int ty = (int)(pc / Wt), tx = (int)(pc - (long long)ty * Wt);
    const Lin ly = lin_index(ty, PP_S, Ht), lx = lin_index(tx, PP_S, Wt);
    const Lin ay0 = lin_index(ly.i0, h, PP_S), ay1 = lin_index(ly.i1, h, PP_S);
    const Lin ax0 = lin_index(lx.i0, w, PP_S), ax1 = lin_index(lx.i1, w, PP_S);
    float best = 0.f;
    int arg = 0;
    for (int k = 0; k < nk; ++k) {
      const float* m = masks + (long long)kq[k] * h * w;
      float v = 0.f;
      if (valid) {
        if (ident) {
          v = sigmoid_at(m, w, ay0, ax0);
        } else {
          const float t0 = sigmoid_at(m, w, ay0, ax0) * lx.l0 + sigmoid_at(m, w, ay0, ax1) * lx.l1;
          const float t1 = sigmoid_at(m, w, ay1, ax0) * lx.l0 + sigmoid_at(m, w, ay1, ax1) * lx.l1;
          v = t0 * ly.l0 + t1 * ly.l1;
        }
        v *= ks[k];
        if (k == 0 || nan_first_gt(v, best)) {
          best = v;
          arg = k;
        }
      }
      const unsigned long long ge = __ballot(valid && v >= mask_threshold);
      if (lane == 0 && ge) atomicAdd(&og[k], __popcll(ge));
    }
    if (valid) {
      seg[p] = arg;
      atomicAdd(&ar[arg], 1);
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < nk; k += 256) {
    if (ar[k]) atomicAdd(&T.area[k], ar[k]);
    if (og[k]) atomicAdd(&T.orig[k], og[k]);
  }
}

struct FuseMask {
  unsigned long long w[PPD_MAX_C / 64];
};

// One workgroup per image, one lane walks the kept queries in order.
__global__ __launch_bounds__(256) void k_pan_assign(int* __restrict__ table, int Q, int C, double overlap,
                                                    FuseMask fuse) {
  __shared__ int mem[PPD_MAX_C];  // the id remembered for a fused label, 0 = not seen
  const PanRow T = pan_row(table, blockIdx.x, Q);
  for (int c = threadIdx.x; c < C; c += 256) mem[c] = 0;
  __syncthreads();
  if (threadIdx.x != 0) return;
  const int nk = *T.nk;
  int cur = 0;
  for (int k = 0; k < nk; ++k) {
    const int area = T.area[k], orig = T.orig[k];
    // torch divides the two int64 counts in float32; .item() is compared as a double
    if (!(area > 0 && orig > 0 && (double)div_rn((float)area, (float)orig) > overlap)) continue;
    const int lab = T.label[k];
    cur = mem[lab] ? mem[lab] : cur + 1;
    T.id[k] = cur;
    if ((fuse.w[lab >> 6] >> (lab & 63)) & 1ull) mem[lab] = cur;
  }
}

// Image b, in place: labels_px -> segment ids; the float32 -1 map when nothing was kept.
__global__ __launch_bounds__(256) void k_pan_paint(const int* __restrict__ table, int b, int Q, long long np,
                                                   int* __restrict__ seg) {
  const int* r = table + (long long)b * (1 + 5 * Q);
  const int nk = r[0];
  for (long long p = blockIdx.x * 256ll + threadIdx.x; p < np; p += 256ll * gridDim.x)
    seg[p] = nk == 0 ? __float_as_int(-1.f) : r[1 + seg[p]];
}

int pixel_grid(long long np, int cap) {
  return (int)std::min<long long>(std::max<long long>(1, (np + 255) / 256), cap);
}

bool sizes_ok(int B, const int* th, const int* tw) {
  for (int b = 0; b < B; ++b)
    if (th[b] <= 0 || tw[b] <= 0) return false;
  return true;
}

}  // namespace

extern "C" {

size_t rgbd_pp_semantic_workspace_size(int B, int Q, int C1) {
  if (B <= 0 || Q <= 0 || C1 < 2) return 256;
  return align256((size_t)B * Q * (C1 - 1) * 4) + align256((size_t)(C1 - 1) * PP_NP * 4);
}

int rgbd_pp_semantic(const float* class_logits, const float* mask_logits, int B, int Q, int C1, int h, int w,
                     const int* target_h_host, const int* target_w_host, long long* const* map_host,
                     float* const* scores_host, void* ws, void* stream) {
  RGBD_REQUIRE(class_logits && mask_logits && target_h_host && target_w_host && map_host && ws, RGBD_E_ARG);
  RGBD_REQUIRE(B > 0 && Q > 0 && C1 >= 2 && h > 0 && w > 0, RGBD_E_ARG);
  RGBD_REQUIRE(C1 - 1 <= PPD_MAX_C, RGBD_E_SHAPE);
  RGBD_REQUIRE(sizes_ok(B, target_h_host, target_w_host), RGBD_E_ARG);
  for (int b = 0; b < B; ++b) RGBD_REQUIRE(map_host[b] && (!scores_host || scores_host[b]), RGBD_E_ARG);
  hipStream_t s = (hipStream_t)stream;
  const int C = C1 - 1;
  float* probs = (float*)ws;
  float* S = (float*)((char*)ws + align256((size_t)B * Q * C * 4));
  k_ppd_softmax<<<ceil_div((long long)B * Q, 256), 256, 0, s>>>(class_logits, B * Q, C1, probs);
  for (int b = 0; b < B; ++b) {  // S holds one image: the launches of one stream run in order
    const int Ht = target_h_host[b], Wt = target_w_host[b];
    k_sem_scores<<<PP_NP / SEM_TP, 256, 0, s>>>(mask_logits + (long long)b * Q * h * w, probs + (long long)b * Q * C, Q,
                                                C, h, w, S);
    k_sem_argmax<<<pixel_grid((long long)Ht * Wt, 4096), 256, 0, s>>>(S, C, Ht, Wt, map_host[b],
                                                                     scores_host ? scores_host[b] : nullptr);
  }
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

size_t rgbd_pp_panoptic_workspace_size(int B, int Q) {
  return B > 0 && Q > 0 ? align256((size_t)B * Q * 4) : 256;
}

int rgbd_pp_panoptic(const float* class_logits, const float* mask_logits, int B, int Q, int C1, int h, int w,
                     const int* target_h_host, const int* target_w_host, double threshold, double mask_threshold,
                     double overlap_mask_area_threshold, const unsigned long long* fuse_mask_host,
                     void* const* seg_host, int* table, void* ws, void* stream) {
  RGBD_REQUIRE(class_logits && mask_logits && target_h_host && target_w_host && seg_host && table && ws, RGBD_E_ARG);
  RGBD_REQUIRE(B > 0 && Q > 0 && C1 >= 2 && h > 0 && w > 0, RGBD_E_ARG);
  RGBD_REQUIRE(C1 - 1 <= PPD_MAX_C && Q <= PPD_MAX_Q, RGBD_E_SHAPE);
  RGBD_REQUIRE(sizes_ok(B, target_h_host, target_w_host), RGBD_E_ARG);
  for (int b = 0; b < B; ++b) RGBD_REQUIRE(seg_host[b], RGBD_E_ARG);
  hipStream_t s = (hipStream_t)stream;
  FuseMask fuse = {};
  if (fuse_mask_host)
    for (int i = 0; i < PPD_MAX_C / 64; ++i) fuse.w[i] = fuse_mask_host[i];
  int* keptq = (int*)ws;
  // the reference compares float32 tensors with its Python thresholds in float32
  k_pan_select<<<B, 256, 0, s>>>(class_logits, Q, C1, (float)threshold, table, keptq);
  for (int b = 0; b < B; ++b) {
    const int Ht = target_h_host[b], Wt = target_w_host[b];
    k_pan_argmax<<<pixel_grid((long long)Ht * Wt, 2048), 256, 0, s>>>(mask_logits + (long long)b * Q * h * w, Q, h, w,
                                                                     keptq, table, b, Ht, Wt, (float)mask_threshold,
                                                                     (int*)seg_host[b]);
  }
  k_pan_assign<<<B, 256, 0, s>>>(table, Q, C1 - 1, overlap_mask_area_threshold, fuse);
  for (int b = 0; b < B; ++b) {
    const long long np = (long long)target_h_host[b] * target_w_host[b];
    k_pan_paint<<<pixel_grid(np, 2048), 256, 0, s>>>(table, b, Q, np, (int*)seg_host[b]);
  }
  RGBD_CHECK_LAUNCH();
  return RGBD_OK;
}

}  // extern "C"
