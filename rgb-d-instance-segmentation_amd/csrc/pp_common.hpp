// Shared by the post-processing kernels (postprocess.hip, postprocess_dense.hip): HF's fixed
// intermediate size and ATen's bilinear index / weight rule.
#pragma once
#include "common.hpp"

namespace rgbd {

constexpr int PP_S = 384;  // HF's fixed intermediate size

// Bilinear source index / weights (ATen compute_source_index_and_lambda, align_corners=False):
// identity at equal sizes, else src = max(scale * (dst + 0.5) - 0.5, 0) with scale = in / out in
// float, i0 = min(floor(src), in - 1), i1 = i0 + (i0 < in - 1), l1 = clamp(src - i0, 0, 1),
// l0 = 1 - l1.  The interpolated value (x inner, y outer, no contraction) agrees with the CPU
// kernel to a few ulp and in sign (oracle/postprocess.py's fixture checks).
struct Lin {
  int i0, i1;
  float l0, l1;
};
__device__ __forceinline__ Lin lin_index(int dst, int in, int out) {
  Lin o;
  if (in == out) {
    o.i0 = o.i1 = dst;
    o.l0 = 1.f;
    o.l1 = 0.f;
    return o;
  }
  const float scale = (float)in / (float)out;
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  o.i0 = min((int)floorf(src), in - 1);
  o.i1 = o.i0 + (o.i0 < in - 1 ? 1 : 0);
  o.l1 = fminf(fmaxf(src - (float)o.i0, 0.f), 1.f);
  o.l0 = 1.f - o.l1;
  return o;
}

}  // namespace rgbd
