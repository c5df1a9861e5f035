// Double-double accumulation shared by the reductions that must not lose what cancels (noise_adj.hip, detscores.hip):
// a sum is carried as an unevaluated pair hi + lo (Knuth's two-sum, the product's error from an fma), ~106 bits.  The
// functions switch floating-point contraction off: a fused multiply-add in place of a rounded product followed by a
// rounded sum would break the error-free transformations (the build uses no fast-math option either).
#pragma once

#include <hip/hip_runtime.h>

namespace psh {

struct dd {
  double hi, lo;
};

__device__ __forceinline__ dd two_sum(double a, double b) {
#pragma clang fp contract(off)
  const double s = a + b;
  const double bb = s - a;
  const double e = (a - (s - bb)) + (b - bb);
  return {s, e};
}
__device__ __forceinline__ dd quick_two_sum(double a, double b) {  // |a| >= |b|
#pragma clang fp contract(off)
  const double s = a + b;
  return {s, b - (s - a)};
}
__device__ __forceinline__ dd dd_add_d(dd a, double b) {
#pragma clang fp contract(off)
  dd t = two_sum(a.hi, b);
  t.lo = t.lo + a.lo;
  return quick_two_sum(t.hi, t.lo);
}
__device__ __forceinline__ dd dd_add(dd a, dd b) {
#pragma clang fp contract(off)
  dd t = two_sum(a.hi, b.hi);
  t.lo = t.lo + (a.lo + b.lo);
  return quick_two_sum(t.hi, t.lo);
}
__device__ __forceinline__ dd dd_add_sq(dd a, double v) {  // a + v * v, the product exact
#pragma clang fp contract(off)
  const double p = v * v;
  const double e = fma(v, v, -p);
  dd t = two_sum(a.hi, p);
  t.lo = t.lo + (a.lo + e);
  return quick_two_sum(t.hi, t.lo);
}
__device__ __forceinline__ dd dd_div_d(dd a, double b) {
#pragma clang fp contract(off)
  const double q1 = a.hi / b;
  const double r = fma(-q1, b, a.hi) + a.lo;
  return quick_two_sum(q1, r / b);
}
__device__ __forceinline__ dd dd_sqr(dd a) {
#pragma clang fp contract(off)
  const double p = a.hi * a.hi;
  const double e = fma(a.hi, a.hi, -p) + 2.0 * (a.hi * a.lo);
  return quick_two_sum(p, e);
}
__device__ __forceinline__ dd dd_wave_sum(dd v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    dd o;
    o.hi = __shfl_xor(v.hi, d);
    o.lo = __shfl_xor(v.lo, d);
    v = dd_add(v, o);
  }
  return v;
}

}  // namespace psh
