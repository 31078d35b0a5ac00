// Pillow's NEAREST resize index rule (Geometry.c affine fast path), shared by the uint8 resize
// (resize.hip) and the RLE painter (rle_decode.hip): xx = 0.5 a0, index = (int)xx, xx += a0 per
// output, a0 = n_in / n_out.  Walked sequentially by one lane: the accumulated double is what
// Pillow indexes with, and at exact integers it can sit one ulp below the product.
#pragma once

namespace rgbd {

__device__ __forceinline__ void pil_nearest_walk(int n_in, int n_out, int* __restrict__ idx) {
  const double a0 = (double)n_in / n_out;
  double xx = 0.5 * a0;
  for (int o = 0; o < n_out; ++o) {
    int v = (int)xx;
    idx[o] = v < 0 ? 0 : (v > n_in - 1 ? n_in - 1 : v);
    xx += a0;
  }
}

}  // namespace rgbd
