// segment_sum.h -- the segmented sum in gather form of texture_fit_kernels.hip (texture_sample_backward_kernel) and
// mesh_fit_kernels.hip (segment_sum_kernel): out[k, :] = the sum over the entries [offsets[k], offsets[k + 1]) of what `add` adds for
// entry e, C floats per row, one lane per segment in blocks of kBlock lanes.  A segment of at most long_segment entries is summed by
// its lane in entry order.  A longer one would leave 63 lanes waiting for one, so it is handed to the whole wavefront by ballot:
// lane l sums entries l, l + 64, ... in entry order, and a fixed shuffle tree combines the 64 partial sums.  No atomics, no LDS, no
// barrier; the additions and their order are a function of the entry list and the threshold alone (tests/segment_sum_model.py
// replays them).  Every row is written, 0 for an empty segment.
#pragma once

#include "rf_device.h"

namespace {

// add(e, acc) adds entry e into acc; it is a template parameter, so the body costs each kernel what its own copy did.  (No
// __restrict__ here: the kernels' own parameters carry it, and a second set of scopes changes the schedule.)
template <int C, int kBlock, typename Add>
__device__ __forceinline__ void segment_sum(const long long* offsets, long long E, long long segments, int long_segment, float* out,
                                            Add add) {
  const long long k = (long long)blockIdx.x * kBlock + threadIdx.x;
  const int lane = (int)(threadIdx.x & 63);
  // (no lane returns early: the ballot loop below needs the whole wavefront)
  long long lo = 0, hi = 0;
  if (k < segments) {  // (clamped: a malformed offset list reads no entry outside [0, E))
    lo = min(max(offsets[k], 0ll), E);
    hi = min(max(offsets[k + 1], lo), E);
  }
  const bool is_long = hi - lo > (long long)long_segment;
  if (k < segments && !is_long) {
    float acc[C] = {};
    for (long long e = lo; e < hi; ++e) add(e, acc);
#pragma unroll
    for (int c = 0; c < C; ++c) out[C * k + c] = acc[c];
  }
  unsigned long long todo = __ballot(is_long);
  while (todo) {  // (wave-uniform)
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const long long slo = __shfl(lo, src, 64), shi = __shfl(hi, src, 64);
    float acc[C] = {};
    for (long long e = slo + lane; e < shi; e += 64) add(e, acc);
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1) {
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] = acc[c] + __shfl_down(acc[c], step, 64);  // (lanes past 63 - step read their own value: only lane 0 is used)
    }
    if (lane == 0) {
      const long long dst = k + src;  // (lane 0's segment is the first of the wavefront's 64)
#pragma unroll
      for (int c = 0; c < C; ++c) out[C * dst + c] = acc[c];
    }
  }
}

}  // namespace
