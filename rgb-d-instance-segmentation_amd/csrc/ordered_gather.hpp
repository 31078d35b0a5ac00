// Ordered segment sums: the second pass of the deterministic (atomic-free) scatters of
// msda.hip and point_loss.hip.
//
// A scatter-add  dst[key[i]] += term[i]  is computed as: (1) an emit pass stores one int32 key
// (the flat destination index, or a sentinel past every destination for a tap that contributes
// nothing) per tap i; (2) the keys are sorted stably carrying i, so the taps of one destination
// form one contiguous segment of the sorted list, in ascending i; (3) every destination finds
// its segment [lo, hi) with two binary searches and sums it in THE ORDER below, which depends on
// the inputs only — never on scheduling:
//
//   the segment is cut into chunks of ORDERED_CH entries at fixed offsets from its start
//   (lo, lo + CH, lo + 2 CH, ...; the last chunk may be shorter);
//   part_k = (((+0 + t_0) + t_1) + ... )   the chunk's terms in ascending sorted position,
//   sum    = (((+0 + part_0) + part_1) + ... )   the partials in chunk order,
//
// every + one float32 addition, every term formed before it is added (no FMA contraction:
// -ffp-contract=off).  An empty segment gives exactly +0.  tests/checkers/ordered_scatter.py
// restates this in numpy float32.
#pragma once

namespace rgbd {

constexpr int ORDERED_CH = 256;

// first position in [lo, n) whose key is >= key (n when there is none); keys ascending
__device__ __forceinline__ int seg_lower_bound(const int* __restrict__ keys, int lo, int n, int key) {
  int hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// the sum of term(j), j in [lo, hi), in the order of this file's header; four terms are formed
// ahead of their additions so that their loads are in flight together
template <int CH, typename F>
__device__ __forceinline__ float ordered_segment_sum(int lo, int hi, F term) {
  float sum = 0.f;
  for (int c0 = lo; c0 < hi; c0 += CH) {
    const int c1 = min(c0 + CH, hi);
    float part = 0.f;
    int j = c0;
    for (; j + 4 <= c1; j += 4) {
      const float t0 = term(j), t1 = term(j + 1), t2 = term(j + 2), t3 = term(j + 3);
      part += t0;
      part += t1;
      part += t2;
      part += t3;
    }
    for (; j < c1; ++j) part += term(j);
    sum += part;
  }
  return sum;
}

}  // namespace rgbd
