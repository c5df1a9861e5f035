// Packed row prefix counts of one or two 0/1 maps (lagprob.hip, fss.hip).
//
// A workgroup of kThreads owns one row of n pixels.  value(x) is a pixel's contribution, one 0/1 bit per 16-bit half
// of a uint32; the row is written as n + 1 words, dst[0] = 0 and dst[x + 1] = sum of value(0 .. x).  Both halves are
// monotone along the row, so a difference of two words of a row never borrows between the halves, and a row of at
// most 65535 pixels never carries.  wave_sum: kThreads / 64 words of LDS.  Every thread of the workgroup calls it.
#pragma once

#include "common.h"

namespace psh {

constexpr int kPackedPrefixMaxWidth = 65535;

template <int kThreads, typename F>
__device__ __forceinline__ void packed_row_prefix(int n, uint32_t *__restrict__ dst, uint32_t *wave_sum, F value) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) dst[0] = 0u;
  uint32_t carry = 0u;
  for (int base = 0; base < n; base += kThreads) {
    const int x = base + tid;
    uint32_t v = x < n ? value(x) : 0u;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t u = __shfl_up(v, d, 64);
      if (lane >= d) v += u;
    }
    if (lane == 63) wave_sum[wave] = v;
    __syncthreads();
    uint32_t before = carry, total = 0u;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) {
      const uint32_t s = wave_sum[w];
      if (w < wave) before += s;
      total += s;
    }
    if (x < n) dst[x + 1] = v + before;
    carry += total;
    __syncthreads();
  }
}

}  // namespace psh
