// K5: DSAM masked 3x3/stride-2 convolutions as MFMA implicit GEMMs (gfx950).
//
// Reference: DSAModule.forward (mask2former/utils/custom_model.py:682-699) evaluates, per
// sample, four Conv3x3s2 on rgb_features * pooled_mask_i plus a bias-free projection conv,
// i.e. five convolutions at batch 1 (and the Python loop of :339-352 repeats it per sample).
// Here one launch covers the whole batch and all five convolutions:
//
//   out[m, n] = sum_{seg<5} sum_{tap<9} sum_{c<Cin} Wseg[n, c, tap] * x[src(m, tap), c] * bit_seg
//
// with K = 5*9*Cin ordered (seg, tap, c): the A operand (im2col of the NHWC input) is loaded
// once per (tap, 32-channel chunk) and re-used by all five segments; segment `seg` < 4 keeps
// an element only where bit `seg` of the pooled region code of its SOURCE pixel is set
// (x * mask, :689).  A segment whose bit is absent from every pixel of a wave's 32 rows is
// skipped (its contribution is exactly zero), which removes most masked FLOPs on real scenes.
//
// dX (training) is the transposed convolution with the same packed structure: output pixels
// are split into the four stride-2 parity classes so only live taps are visited, and the
// mask bit is taken at the OUTPUT pixel (d(x*m)/dx = m).  dW contracts over pixels with an
// LDS-staged im2col tile.
//
// That is the float32 form.  bf16 regroups the sum by region code (one merged filter per code
// instead of popcount + 1 segments per pixel) and runs persistent LDS-DMA kernels over plans built
// on the device from the region codes; see dsam_lds.hip and dsam_wgrad.hip.
//
// Files: this one holds the C ABI of the legs: it validates the arguments, fills the launch
// arguments and calls the leg files' launch functions (dsam_common.hpp).  The kernels, their tile
// constants, grids and plan / workspace arithmetic are in
//   dsam_pack.hip   k_pack_dsam, k_pack_codes, k_code_masks (and their C entry points)
//   dsam_f32.hip    k_conv_igemm (forward, dX); k_dsam_wgrad -> k_chan_sum<float> ->
//                   k_dsam_wgrad_final -> k_dsam_bias_grad (dW)
//   dsam_lds.hip    plan: k_dsam_plan -> k_dsam_items; run: k_dsam_lds<KC, ...> (forward, dX)
//   dsam_wgrad.hip  plan: k_code_presence_legs -> k_wg_plan_legs -> k_wg_masks_legs;
//                   run: k_dsam_wgrad_mm<FM, legs> (-> k_chan_sum<bf16_t> given an NCHW gradient)
//                   -> k_dsam_wgrad_fold
// The NCHW -> NHWC converters that feed these legs are in layout.hip.
#include "dsam_common.hpp"

using namespace rgbd;
using namespace rgbd::k5;

namespace {

ConvArgs fwd_args(int B, int Cin, int h, int w, int Cout) {
  ConvArgs a = {};
  a.B = B; a.Hi = h; a.Wi = w; a.C = Cin;
  a.Ho = (h + 1) / 2; a.Wo = (w + 1) / 2; a.N = Cout;
  a.KH = 3; a.KW = 3; a.stride = 2; a.pad = 1;
  a.nseg = 5; a.mask_mode = MASK_SRC; a.transposed = 0;
  return a;
}
ConvArgs dx_args(int B, int Cin, int h, int w, int Cout) {
  ConvArgs a = {};
  a.B = B; a.Hi = (h + 1) / 2; a.Wi = (w + 1) / 2; a.C = Cout;
  a.Ho = h; a.Wo = w; a.N = Cin;
  a.KH = 3; a.KW = 3; a.stride = 2; a.pad = 1;
  a.nseg = 5; a.mask_mode = MASK_DST; a.transposed = 1;
  return a;
}
ConvArgs leg_conv_args(const rgbd_dsam_leg& g) {
  ConvArgs a = g.kind == RGBD_LEG_FWD ? fwd_args(g.B, g.Cin, g.h, g.w, g.Cout) : dx_args(g.B, g.Cin, g.h, g.w, g.Cout);
  a.code = g.code;
  return a;
}
bool leg_ok(const rgbd_dsam_leg& g) {
  return (g.kind == RGBD_LEG_FWD || g.kind == RGBD_LEG_DX || g.kind == RGBD_LEG_DW) && g.B > 0 && g.h > 0 &&
         g.w > 0 && g.Cin > 0 && g.Cout > 0;
}

}  // namespace

extern "C" {

int rgbd_dsam_fwd(int dtype, const void* x_nhwc, const uint8_t* code, const rgbd_decomp_info* info,
                  int B, int Cin, int h, int w, int Cout, const void* wfwd, const float* bias,
                  const void* residual, void* out_nchw, void* out_nhwc, const void* plan, void* ws,
                  void* stream) {
  RGBD_REQUIRE(!plan || dtype == RGBD_BF16, RGBD_E_DTYPE);
  RGBD_REQUIRE(x_nhwc && code && info && wfwd && bias && (out_nchw || out_nhwc), RGBD_E_ARG);
  RGBD_REQUIRE(B > 0 && h > 0 && w > 0 && Cout > 0 && Cin > 0, RGBD_E_ARG);
  RGBD_REQUIRE(Cin % 8 == 0, RGBD_E_SHAPE);
  ConvArgs a = fwd_args(B, Cin, h, w, Cout);
  a.x = x_nhwc; a.code = code; a.w = wfwd;
  a.bias4 = bias; a.info = info; a.residual = residual; a.out_nchw = out_nchw; a.out_nhwc = out_nhwc;
  a.partial = (float*)ws;
  RGBD_REQUIRE((plan && ws) || dtype != RGBD_BF16, RGBD_E_ARG);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == RGBD_F32) return conv_f32(a, s);
  if (dtype == RGBD_BF16) return conv_bf16(a, plan, s);
  return RGBD_E_DTYPE;
}

int rgbd_dsam_fwd_nhwc(int dtype, const void* x_nhwc, const uint8_t* code, const rgbd_decomp_info* info, int B,
                       int Cin, int h, int w, int Cout, const void* wfwd, const float* bias,
                       const void* residual_nhwc, void* out_nhwc, const float* residual_f32_nhwc,
                       float* out_f32_nhwc, const void* plan, void* ws, void* stream) {
  RGBD_REQUIRE(dtype == RGBD_BF16, RGBD_E_DTYPE);
  RGBD_REQUIRE(x_nhwc && code && info && wfwd && bias && (out_nhwc || out_f32_nhwc) && plan && ws, RGBD_E_ARG);
  RGBD_REQUIRE(B > 0 && h > 0 && w > 0 && Cout > 0 && Cin > 0, RGBD_E_ARG);
  // the float32-interface kernel takes its residual as float32 only
  RGBD_REQUIRE(!((residual_f32_nhwc || out_f32_nhwc) && residual_nhwc), RGBD_E_ARG);
  RGBD_REQUIRE((((uintptr_t)residual_f32_nhwc | (uintptr_t)out_f32_nhwc) & 15) == 0, RGBD_E_ARG);  // 16-byte accesses
  ConvArgs a = fwd_args(B, Cin, h, w, Cout);
  a.x = x_nhwc; a.code = code; a.w = wfwd;
  a.bias4 = bias; a.info = info; a.residual_nhwc = residual_nhwc; a.out_nhwc = out_nhwc;
  a.residual_f32_nhwc = residual_f32_nhwc; a.out_f32_nhwc = out_f32_nhwc;
  a.partial = (float*)ws;
  return conv_bf16(a, plan, (hipStream_t)stream);
}

int rgbd_dsam_bwd_data(int dtype, const void* gout_nhwc, const uint8_t* code, int B, int Cin, int h, int w,
                       int Cout, const void* wbwd, const void* gin_nchw, const void* gin_nhwc, void* dx_nchw,
                       void* dx_nhwc, const void* plan, void* ws, void* stream) {
  RGBD_REQUIRE(!plan || dtype == RGBD_BF16, RGBD_E_DTYPE);
  RGBD_REQUIRE(gout_nhwc && code && wbwd && (dx_nchw || dx_nhwc), RGBD_E_ARG);
  // the residual comes in the layout of the pass that adds it: NCHW with an NCHW output, NHWC
  // (bf16 only) without one
  RGBD_REQUIRE(!gin_nhwc || (dtype == RGBD_BF16 && !dx_nchw && !gin_nchw), RGBD_E_ARG);
  RGBD_REQUIRE(!gin_nchw || dx_nchw, RGBD_E_ARG);
  RGBD_REQUIRE(B > 0 && h > 0 && w > 0 && Cout > 0 && Cin > 0, RGBD_E_ARG);
  RGBD_REQUIRE(Cout % 8 == 0, RGBD_E_SHAPE);
  ConvArgs a = dx_args(B, Cin, h, w, Cout);
  a.x = gout_nhwc; a.code = code; a.w = wbwd;
  a.residual = gin_nchw; a.residual_nhwc = gin_nhwc; a.out_nchw = dx_nchw; a.out_nhwc = dx_nhwc;
  a.partial = (float*)ws;
  RGBD_REQUIRE((plan && ws) || dtype != RGBD_BF16, RGBD_E_ARG);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == RGBD_F32) return conv_f32(a, s);
  if (dtype == RGBD_BF16) return conv_bf16(a, plan, s);
  return RGBD_E_DTYPE;
}

int rgbd_dsam_bwd_weight(int dtype, const void* gout_nchw, const void* gout_nhwc, const void* x_nhwc,
                         const uint8_t* code, const rgbd_decomp_info* info, int B, int Cin, int h, int w,
                         int Cout, float* dconv_w, float* dproj_w, float* dbias, const void* plan, void* ws,
                         void* stream) {
  RGBD_REQUIRE(!plan || dtype == RGBD_BF16, RGBD_E_ARG);
  RGBD_REQUIRE((gout_nchw || dtype == RGBD_BF16) && x_nhwc && code && info && dconv_w && dproj_w && dbias && ws,
               RGBD_E_ARG);
  RGBD_REQUIRE(B > 0 && h > 0 && w > 0 && Cout > 0 && Cin > 0, RGBD_E_ARG);
  RGBD_REQUIRE(Cin % 8 == 0, RGBD_E_SHAPE);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == RGBD_BF16) {
    RGBD_REQUIRE(gout_nhwc && plan, RGBD_E_ARG);
    const rgbd_dsam_dw_run r = {gout_nhwc, x_nhwc, code, B, Cin, h, w, Cout, dconv_w, dproj_w, dbias, plan, ws};
    return wgrad_bf16(1, &r, gout_nchw, info, s);
  }
  if (dtype != RGBD_F32) return RGBD_E_DTYPE;
  return wgrad_f32((const float*)gout_nchw, (const float*)x_nhwc, code, info, B, Cin, h, w, Cout, dconv_w, dproj_w,
                   dbias, ws, s);
}

int rgbd_dsam_bwd_weight_multi(int n, const rgbd_dsam_dw_run* runs, const rgbd_decomp_info* info, void* stream) {
  RGBD_REQUIRE(n >= 1 && n <= 2 && runs && info, RGBD_E_ARG);
  for (int i = 0; i < n; ++i) {
    const rgbd_dsam_dw_run& r = runs[i];
    RGBD_REQUIRE(r.gout_nhwc && r.x_nhwc && r.code && r.dconv_w && r.dproj_w && r.dbias && r.plan && r.ws, RGBD_E_ARG);
    RGBD_REQUIRE(r.B > 0 && r.h > 0 && r.w > 0 && r.Cout > 0 && r.Cin > 0 && r.Cin % 8 == 0, RGBD_E_SHAPE);
    RGBD_REQUIRE(wgrad_shape_ok(r.B, r.Cin, r.h, r.w, r.Cout), RGBD_E_SHAPE);
  }
  for (int i = 0; i + 1 < n; ++i)  // distinct buffers: the legs run together
    RGBD_REQUIRE(runs[i].ws != runs[i + 1].ws && runs[i].plan != runs[i + 1].plan, RGBD_E_ARG);
  return wgrad_bf16(n, runs, nullptr, info, (hipStream_t)stream);
}

// ---- planning ahead (bf16): the code-dependent set-up of a leg depends only on the region codes,
// so the hot path plans every leg of the step once, right after the decomposition
size_t rgbd_dsam_plan_size(int kind, int B, int Cin, int h, int w, int Cout) {
  const rgbd_dsam_leg g = {kind, nullptr, B, Cin, h, w, Cout, nullptr};
  if (!leg_ok(g)) return 0;
  if (kind == RGBD_LEG_DW) return wgrad_plan_bytes(B, Cin, h, w, Cout);
  return conv_plan_bytes(leg_conv_args(g));
}
size_t rgbd_dsam_run_workspace_size(int dtype, int kind, int B, int Cin, int h, int w, int Cout) {
  const rgbd_dsam_leg g = {kind, nullptr, B, Cin, h, w, Cout, nullptr};
  if (!leg_ok(g) || (dtype != RGBD_BF16 && dtype != RGBD_F32)) return 0;
  if (kind == RGBD_LEG_DW)
    return dw_run_ws(dtype == RGBD_BF16 ? wgrad_partial_elems(B, Cin, h, w, Cout) : wgrad_f32_partial_elems(B, Cin, Cout),
                     B, Cout)
        .total;
  if (dtype == RGBD_F32) return 256;  // the float32 forward / dX use no workspace
  return std::max<size_t>(256, conv_partial_bytes(leg_conv_args(g)));
}

int rgbd_dsam_plan(int n, const rgbd_dsam_leg* legs, void* stream) {
  RGBD_REQUIRE(n > 0 && legs, RGBD_E_ARG);
  hipStream_t s = (hipStream_t)stream;
  ConvArgs conv[PLAN_MAXLEG];
  void* conv_plans[PLAN_MAXLEG];
  rgbd_dsam_leg dw[WG_MAXLEG];
  int nconv = 0, ndw = 0;
  for (int i = 0; i < n; ++i) {  // every leg is checked before anything is launched
    const rgbd_dsam_leg& g = legs[i];
    RGBD_REQUIRE(leg_ok(g) && g.code && g.plan, RGBD_E_ARG);
    if (g.kind == RGBD_LEG_DW) {
      RGBD_REQUIRE(ndw < WG_MAXLEG, RGBD_E_ARG);
      RGBD_REQUIRE(wgrad_shape_ok(g.B, g.Cin, g.h, g.w, g.Cout), RGBD_E_SHAPE);
      dw[ndw++] = g;
      continue;
    }
    RGBD_REQUIRE(nconv < PLAN_MAXLEG, RGBD_E_ARG);
    conv[nconv] = leg_conv_args(g);
    RGBD_REQUIRE(conv_shape_ok(conv[nconv]), RGBD_E_SHAPE);
    conv_plans[nconv++] = g.plan;
  }
  if (nconv) {
    const int rc = conv_plan(nconv, conv, conv_plans, s);
    if (rc != RGBD_OK) return rc;
  }
  if (ndw) return wgrad_plan(ndw, dw, s);
  return RGBD_OK;
}

}  // extern "C"
