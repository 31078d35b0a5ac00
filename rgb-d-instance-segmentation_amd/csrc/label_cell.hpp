// The id a label-map cell names, shared by the overlay blend and the segment matcher.
#pragma once
#include "common.hpp"

namespace rgbd {

// the id a map cell names, or -1: float32 cells name an id only when they hold that integer exactly
// (the reference compares the map with == against the integer id)
template <bool F32>
__device__ __forceinline__ int cell_id(uint32_t bits, int n_ids) {
  if constexpr (F32) {
    const float f = __uint_as_float(bits);
    if (!(f >= 0.f && f < (float)n_ids)) return -1;  // NaN lands here too
    const int i = (int)f;
    return (float)i == f ? i : -1;
  } else {
    const int i = (int)bits;
    return (i >= 0 && i < n_ids) ? i : -1;
  }
}

}  // namespace rgbd
