// What the deterministic-score kernels share (detscores.hip: a forecast against its observation; ensscores.hip: all
// pairs of an ensemble's members): the walk of a member in chunks of four pixels, the grid that walk is cut into and the
// one double-double term that dd.h does not have.  The pair sums of ensscores.hip are held to those of detscores.hip bit
// for bit, so the order of a sum - chunk c to thread c % (groups * kDetThreads), kDetMaxGroups - lives here once.
#pragma once

#include <cstddef>
#include <cstdint>

#include "dd.h"

namespace psh {

constexpr int kDetThreads = 256;
constexpr int kDetMaxGroups = 512;  // workgroups per member - fixed: the summation order is part of the result

// the sums over the pairs, in the order both files return them
enum { kSumRes = 0, kSumRes2, kSumAbs, kSumSum2, kSumObsPair, kSumPredPair, kSumObsPred, kPairSums };

__device__ __forceinline__ double quiet_nan() { return __builtin_nan(""); }

// four consecutive pixels from element i (a multiple of 4) as float64; beyond npix: NaN (counts nowhere)
__device__ __forceinline__ void load4(const float *__restrict__ p, size_t i, size_t npix, bool vec, double (&x)[4]) {
  if (vec && i + 4 <= npix) {
    const float4 v = *reinterpret_cast<const float4 *>(p + i);
    x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = i + j < npix ? static_cast<double>(p[i + j]) : quiet_nan();
  }
}
__device__ __forceinline__ void load4(const double *__restrict__ p, size_t i, size_t npix, bool vec, double (&x)[4]) {
  if (vec && i + 4 <= npix) {
    const double2 a = *reinterpret_cast<const double2 *>(p + i);
    const double2 b = *reinterpret_cast<const double2 *>(p + i + 2);
    x[0] = a.x, x[1] = a.y, x[2] = b.x, x[3] = b.y;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = i + j < npix ? p[i + j] : quiet_nan();
  }
}

template <typename T>
__device__ __forceinline__ bool aligned16(const T *p) {
  return (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
}

__device__ __forceinline__ dd dd_add_prod(dd a, double x, double y) {  // a + x * y, the product exact
#pragma clang fp contract(off)
  const double p = x * y;
  const double e = fma(x, y, -p);
  dd t = two_sum(a.hi, p);
  t.lo = t.lo + (a.lo + e);
  return quick_two_sum(t.hi, t.lo);
}

inline int det_groups(size_t npix) {
  const size_t chunks = (npix + 3) / 4, groups = (chunks + kDetThreads - 1) / kDetThreads;
  return static_cast<int>(groups < static_cast<size_t>(kDetMaxGroups) ? groups : kDetMaxGroups);
}

}  // namespace psh
