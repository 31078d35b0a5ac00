// K5 (the DSAM masked convolutions) internals shared by dsam_conv.hip and its leg files
// dsam_{pack,f32,lds,wgrad}.hip: the conv launch arguments, the few constants more than one file
// needs, and the leg files' host launch, plan and sizing functions.  The overview of what runs
// when is at the top of dsam_conv.hip.
#pragma once
#include <algorithm>

#include "mfma.hpp"
#include "timing.hpp"

namespace rgbd::k5 {

enum { MASK_NONE = 0, MASK_SRC = 1, MASK_DST = 2 };

// One conv leg, forward or dX (dsam_f32.hip: k_conv_igemm; dsam_lds.hip: k_dsam_lds and its plan
// kernels, which use the fields marked bf16)
struct ConvArgs {
  const void* x;          // NHWC [B][Hi][Wi][C]
  const uint8_t* code;    // region codes: [B][Hi][Wi] (MASK_SRC) or [B][Ho][Wo] (MASK_DST)
  const void* w;          // packed B operand [N][nseg * KH*KW * C]
  int B, Hi, Wi, C;
  int Ho, Wo, N;
  int KH, KW, stride, pad;
  int nseg, mask_mode, transposed;
  const float* bias4;               // DSAM conv biases [4][N] (summed over i < n_masks[b])
  const rgbd_decomp_info* info;
  const void* residual;             // NCHW [B][N][Ho][Wo] added in the epilogue (optional)
  const void* residual_nhwc;        // bf16 only: NHWC residual, used when out_nchw is null
  void* out_nchw;                   // optional
  void* out_nhwc;                   // optional
  int linear;                       // bf16: tile rows = 128 consecutive pixels of the (class) grid
                                    // over the batch instead of 8 x 16 blocks (small grids)
  uint16_t* tmasks;                 // bf16: [class][tile][16] per-tap code sets (k_dsam_plan)
  int* items;                       // bf16: work list of k_dsam_lds (k_dsam_items)
  int* nitems;
  int* tickets;                     // bf16: per (class, tile, N tile) chunk counter, zeroed by k_dsam_plan
  int* work;                        // bf16: per N tile next-item counter of k_dsam_lds, zeroed by k_dsam_plan
  int ntiles0;                      // bf16: tiles of the largest class
  int chunk_len;                    // bf16: steps per workgroup chunk of a tile
  int ncg;                          // bf16: K chunk groups per tap (C / (32 * KC))
  float* partial;                   // bf16: partial tiles of multi-chunk tiles (reduced by their last chunk)
  const bf16_t* zero;               // bf16: LD_ZERO_BYTES of zeros (zeroed by k_dsam_plan)
  unsigned long long* stamps;       // diagnostics only (rgbd_debug_dsam_stamps); null otherwise
  // the F32IO instantiation of k_dsam_lds only (forward, NHWC-only epilogue):
  const float* residual_f32_nhwc;   // optional float32 NHWC residual (instead of residual_nhwc)
  float* out_f32_nhwc;              // optional float32 NHWC copy of the result before its rounding
};

// rows of the implicit GEMM (of the largest stride-2 parity class for dX)
inline long long conv_mmax(const ConvArgs& a) {
  return a.transposed ? (long long)a.B * ((a.Ho + 1) / 2) * ((a.Wo + 1) / 2) : (long long)a.B * a.Ho * a.Wo;
}

constexpr int LD_ZERO_BYTES = 512;  // zeroed global row the DMA reads for masked-out operand rows
                                    // (the tail of every bf16 plan buffer, conv and dW)
constexpr int PLAN_MAXLEG = 8;      // conv legs one rgbd_dsam_plan call takes
constexpr int WG_MAXLEG = 4;        // dW legs it takes
constexpr int CS_SPLIT_MAX = 16;    // pixel ranges of a bf16 dW leg's NHWC channel sums

// lds_swz: 16-byte chunk g of 64-byte row n sits at slot g ^ lds_swz(n), in the packed bf16 filters
// (k_pack_codes) as in the LDS image k_dsam_lds copies them to.  A fragment read has
// lane (r, g) take chunk g of row base+r (base a multiple of 16); the slot is 4*(n%4) + chunk, and
// with the XOR by 2 on rows 8..15 of every 16 the 16 lanes of each ds_read_b128 lane group
// ({0-3,12-15,20-27}, {4-11,16-19,28-31}, ...; MI355X_MICROARCH.md LDS table) hit 16 distinct
// 4-bank slots: conflict-free.  (The earlier (n >> 2) & 3 was conflict-free only for 16
// consecutive lanes, not for the hardware groups.)
__host__ __device__ __forceinline__ int lds_swz(int n) { return ((n >> 3) & 1) << 1; }

// The bias channel sums of an NCHW upstream gradient: k_chan_sum<float> in dsam_f32.hip,
// k_chan_sum<bf16_t> in dsam_wgrad.hip (a bf16 dW given one).  Anonymous namespace, like every
// kernel of the leg files: each file's instantiation is its own, and the library exports neither.
namespace {
template <typename T>
__global__ __launch_bounds__(256) void k_chan_sum(const T* __restrict__ g, int HW, float* __restrict__ out) {
  // out[b*C + c] = sum_p g[b][c][p]   (one block per (b, c))
  __shared__ float red[4];
  const long long base = (long long)blockIdx.x * HW;
  float s = 0.f;
  for (int p = threadIdx.x; p < HW; p += 256) s += Num<T>::to_f(g[base + p]);
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}
}  // namespace

// dW run workspace of either precision: [partials f32 (bf16: [items][Cout][9 Cin]; float32:
// [splits][Cout][45 Cin]) | channel sums]
struct DwRunWs {
  size_t csum, total;  // the partials start the workspace
};
inline DwRunWs dw_run_ws(size_t partial_elems, int B, int Cout) {
  DwRunWs o;
  o.csum = align256(sizeof(float) * partial_elems);
  o.total = o.csum + align256(sizeof(float) * (size_t)CS_SPLIT_MAX * B * Cout);
  return o;
}

// ------------------------------------------------------------------ leg launch functions
// Each launches its leg's kernels on stream s and returns RGBD_OK, an RGBD_E_* code or a HIP error.

// dsam_f32.hip: the float32 segment-form path.  Forward / dX ("dsam_fwd" / "dsam_dx" timer scopes)
// use no plan and no workspace; dW ("dsam_wgrad") the run workspace dw_run_ws(wgrad_f32_partial_elems)
int conv_f32(const ConvArgs& a, hipStream_t s);
size_t wgrad_f32_partial_elems(int B, int Cin, int Cout);
int wgrad_f32(const float* gout_nchw, const float* x_nhwc, const uint8_t* code, const rgbd_decomp_info* info, int B,
              int Cin, int h, int w, int Cout, float* dconv_w, float* dproj_w, float* dbias, void* ws, hipStream_t s);

// dsam_lds.hip: the bf16 code-merged forward / dX (same timer scopes).  A leg's plan buffer is
// conv_plan_bytes, written by conv_plan (n <= PLAN_MAXLEG legs, plans[i] the buffer of legs[i]);
// conv_bf16 runs a planned leg, its partial-tile buffer a.partial conv_partial_bytes
bool conv_shape_ok(const ConvArgs& a);
size_t conv_plan_bytes(const ConvArgs& a);
size_t conv_partial_bytes(const ConvArgs& a);
int conv_plan(int n, const ConvArgs* legs, void* const* plans, hipStream_t s);
int conv_bf16(const ConvArgs& a, const void* plan, hipStream_t s);

// dsam_wgrad.hip: the bf16 code-merged dW ("dsam_wgrad" scope).  A leg's plan buffer is
// wgrad_plan_bytes, written by wgrad_plan (n <= WG_MAXLEG legs of kind RGBD_LEG_DW); its run
// workspace dw_run_ws(wgrad_partial_elems).  wgrad_bf16 runs n = 1 | 2 planned legs: two legs of one
// output tile shape share a GEMM launch, and both legs' folds are one launch.  gout_nchw (n = 1 only,
// optional): the same upstream gradient as NCHW, which the bias channel sums then read.
bool wgrad_shape_ok(int B, int Cin, int h, int w, int Cout);
size_t wgrad_plan_bytes(int B, int Cin, int h, int w, int Cout);
size_t wgrad_partial_elems(int B, int Cin, int h, int w, int Cout);
int wgrad_plan(int n, const rgbd_dsam_leg* legs, hipStream_t s);
int wgrad_bf16(int n, const rgbd_dsam_dw_run* runs, const void* gout_nchw, const rgbd_decomp_info* info,
               hipStream_t s);

}  // namespace rgbd::k5
