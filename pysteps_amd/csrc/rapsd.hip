// Radially averaged power spectral density on gfx950: pysteps/utils/spectral.py:100-180 (rapsd) for a stack of K
// planes.  Every coefficient (ky, kx) belongs to the bin r = round(sqrt(kx^2 + ky^2)); the result is the mean of the
// power over each bin r < nb, with l = max(m, n) and nb = l / 2 (+ 1 for odd l).
//
// The bin is an integer function of N = kx^2 + ky^2: r is the integer with r^2 - r < N <= r^2 + r (r = 0 for N = 0),
// since sqrt(N) is never a half-integer.  Turned round, the coefficients of bin r in the row ky are those with
// r^2 - r - ky^2 < kx^2 <= r^2 + r - ky^2: one run of |kx|.  That gives a gather with no scatter and no atomics:
//
//   rapsd_partial   thread r of row group g walks the rows g, g + G, ... and adds the run of its bin in each row, in
//                   column order, into double-double pairs (dd.h).  Neighbouring threads own neighbouring bins, whose
//                   runs are neighbouring columns of the row.  One partial per (plane, group, bin).
//                     half spectrum (m, n/2+1) complex128 as psh_fft_rfft2_dev writes it: row i is ky = i or i - m,
//                       column c is kx = c; re^2 + im^2 without a rounding (fma); the columns 0 and, for even n, n/2
//                       stand for themselves, every other column for itself and its mirror (weight 2), which makes
//                       sums and counts those of the full plane.
//                     full shifted plane (m, n) float32 or float64: row i is ky = i - m/2, column j is kx = j - n/2;
//                       the run lies on both sides of the centre column.
//   rapsd_finish    thread r adds the G partials in group order and divides by the bin's count (and by m n for the
//                   half spectrum) in double-double; one rounding to float64.
//   rapsd_count     the bin counts as integers from the same runs; a function of the shape.
// G and the walk depend on the shape alone, so a plane's spectrum is the same bits in every run, for every K and at
// every position in a stack.
#include "common.h"
#include "dd.h"

namespace psh {
namespace {

constexpr int kRapsdThreads = 256;
constexpr int kRapsdMaxGroups = 32;  // row groups per plane - fixed: the summation order is part of the result

__device__ __forceinline__ int isqrt_floor(long long v) {  // v >= 0, < 2^40
  int s = static_cast<int>(sqrt(static_cast<double>(v)));
  while (static_cast<long long>(s) * s > v) --s;
  while (static_cast<long long>(s + 1) * (s + 1) <= v) ++s;
  return s;
}

// the run lo..hi of |kx| that bin r takes in the row ky; false when it is empty
__device__ __forceinline__ bool bin_run(int r, int ky, int &lo, int &hi) {
  const long long k2 = static_cast<long long>(ky) * ky, r2 = static_cast<long long>(r) * r;
  if (r == 0) {
    lo = hi = 0;
    return ky == 0;
  }
  const long long upper = r2 + r - k2;  // kx^2 <= upper
  if (upper < 0) return false;
  const long long below = r2 - r - k2;  // kx^2 > below
  hi = isqrt_floor(upper);
  lo = below < 0 ? 0 : isqrt_floor(below) + 1;
  return lo <= hi;
}

__host__ __device__ __forceinline__ int rapsd_bins(int m, int n) {
  const int l = m > n ? m : n;
  return l / 2 + (l & 1);
}

__device__ __forceinline__ dd dd_scale2(dd a) { return {2.0 * a.hi, 2.0 * a.lo}; }

// grid (ceil(nb / threads), G, K); partial (K, G, nb)
__global__ __launch_bounds__(kRapsdThreads) void rapsd_partial_half(const double2 *__restrict__ spec, int m, int n, int nb,
                                                                     dd *__restrict__ partial) {
#pragma clang fp contract(off)
  const int r = blockIdx.x * kRapsdThreads + threadIdx.x;
  if (r >= nb) return;
  const int nh = n / 2 + 1, G = gridDim.y, g = blockIdx.y;
  const int nyq = (n & 1) ? -1 : n / 2;  // the column that has no mirror besides column 0
  const double2 *plane = spec + static_cast<size_t>(blockIdx.z) * m * nh;
  dd own = {0.0, 0.0}, twice = {0.0, 0.0};
  for (int i = g; i < m; i += G) {
    const int ky = i <= (m - 1) / 2 ? i : i - m;
    int lo, hi;
    if (!bin_run(r, ky, lo, hi)) continue;
    if (hi > nh - 1) hi = nh - 1;
    const double2 *row = plane + static_cast<size_t>(i) * nh;
    for (int c = lo; c <= hi; ++c) {
      const double2 v = row[c];
      if (c == 0 || c == nyq) {
        own = dd_add_sq(own, v.x);
        own = dd_add_sq(own, v.y);
      } else {
        twice = dd_add_sq(twice, v.x);
        twice = dd_add_sq(twice, v.y);
      }
    }
  }
  partial[(static_cast<size_t>(blockIdx.z) * G + g) * nb + r] = dd_add(own, dd_scale2(twice));
}

template <typename T>
__global__ __launch_bounds__(kRapsdThreads) void rapsd_partial_full(const T *__restrict__ planes, int m, int n, int nb,
                                                                     dd *__restrict__ partial) {
#pragma clang fp contract(off)
  const int r = blockIdx.x * kRapsdThreads + threadIdx.x;
  if (r >= nb) return;
  const int G = gridDim.y, g = blockIdx.y, cy = m / 2, cx = n / 2;
  const T *plane = planes + static_cast<size_t>(blockIdx.z) * m * n;
  dd acc = {0.0, 0.0};
  for (int i = g; i < m; i += G) {
    int lo, hi;
    if (!bin_run(r, i - cy, lo, hi)) continue;
    const T *row = plane + static_cast<size_t>(i) * n;
    const int hi_neg = hi < cx ? hi : cx;  // kx = -x is column cx - x >= 0
    for (int x = hi_neg; x >= (lo > 1 ? lo : 1); --x) acc = dd_add_d(acc, static_cast<double>(row[cx - x]));
    const int hi_pos = hi < n - 1 - cx ? hi : n - 1 - cx;  // kx = x is column cx + x <= n - 1
    for (int x = lo; x <= hi_pos; ++x) acc = dd_add_d(acc, static_cast<double>(row[cx + x]));
  }
  partial[(static_cast<size_t>(blockIdx.z) * G + g) * nb + r] = acc;
}

// grid (ceil(nb / threads)); shifted != 0: the rows and columns of the full shifted plane, else those of the half
// spectrum with its weights - the same numbers, both kept so that the tests can say so
__global__ __launch_bounds__(kRapsdThreads) void rapsd_count(int m, int n, int nb, int shifted,
                                                              unsigned long long *__restrict__ counts) {
  const int r = blockIdx.x * kRapsdThreads + threadIdx.x;
  if (r >= nb) return;
  const int cx = n / 2, cy = m / 2, nh = n / 2 + 1, nyq = (n & 1) ? -1 : n / 2;
  unsigned long long total = 0ull;
  for (int i = 0; i < m; ++i) {
    int lo, hi;
    if (shifted) {
      if (!bin_run(r, i - cy, lo, hi)) continue;
      const int hi_neg = hi < cx ? hi : cx, lo_neg = lo > 1 ? lo : 1, hi_pos = hi < n - 1 - cx ? hi : n - 1 - cx;
      if (hi_neg >= lo_neg) total += hi_neg - lo_neg + 1;
      if (hi_pos >= lo) total += hi_pos - lo + 1;
    } else {
      if (!bin_run(r, i <= (m - 1) / 2 ? i : i - m, lo, hi)) continue;
      if (hi > nh - 1) hi = nh - 1;
      if (hi < lo) continue;
      total += 2ull * (hi - lo + 1);
      if (lo == 0) total -= 1ull;
      if (lo <= nyq && nyq <= hi) total -= 1ull;
    }
  }
  counts[r] = total;
}

// grid (ceil(nb / threads), K)
__global__ __launch_bounds__(kRapsdThreads) void rapsd_finish(const dd *__restrict__ partial, int G, int nb,
                                                               const unsigned long long *__restrict__ counts, double scale,
                                                               double *__restrict__ out) {
#pragma clang fp contract(off)
  const int r = blockIdx.x * kRapsdThreads + threadIdx.x;
  if (r >= nb) return;
  const dd *src = partial + static_cast<size_t>(blockIdx.y) * G * nb + r;
  dd t = src[0];
  for (int g = 1; g < G; ++g) t = dd_add(t, src[static_cast<size_t>(g) * nb]);
  const dd q = dd_div_d(t, static_cast<double>(counts[r]) * scale);  // count * m * n < 2^53: exact
  out[static_cast<size_t>(blockIdx.y) * nb + r] = q.hi + q.lo;
}

template <typename T>
__global__ __launch_bounds__(kRapsdThreads) void rapsd_nonfinite(const T *__restrict__ in, size_t count,
                                                                  unsigned long long *__restrict__ out) {
  unsigned nan = 0u, inf = 0u;
  const size_t stride = static_cast<size_t>(gridDim.x) * kRapsdThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kRapsdThreads + threadIdx.x; i < count; i += stride) {
    const double v = static_cast<double>(in[i]);
    nan += v != v ? 1u : 0u;
    inf += __builtin_isinf(v) ? 1u : 0u;
  }
  if (nan) atomicAdd(out, static_cast<unsigned long long>(nan));  // integer adds commute
  if (inf) atomicAdd(out + 1, static_cast<unsigned long long>(inf));
}

// out = in widened, NaN replaced by `fill`
template <typename T>
__global__ __launch_bounds__(kRapsdThreads) void rapsd_fill_nan(const T *__restrict__ in, size_t count, double fill,
                                                                 double *__restrict__ out) {
  const size_t stride = static_cast<size_t>(gridDim.x) * kRapsdThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kRapsdThreads + threadIdx.x; i < count; i += stride) {
    const double v = static_cast<double>(in[i]);
    out[i] = v != v ? fill : v;
  }
}

int check_shape(const char *what, int K, int m, int n) {
  if (m < 1 || n < 1 || m > 16384 || n > 16384) return fail(PSH_EINVAL, "%s: shape (%d, %d) (sides 1..16384)", what, m, n);
  if (K < 1 || K > 65535) return fail(PSH_EINVAL, "%s: %d planes (1..65535)", what, K);
  return PSH_OK;
}

int groups_for(int m) { return m < kRapsdMaxGroups ? m : kRapsdMaxGroups; }

int launch_count(int m, int n, int shifted, unsigned long long *counts_dev, hipStream_t s) {
  const int nb = rapsd_bins(m, n);
  hipLaunchKernelGGL(rapsd_count, dim3((nb + kRapsdThreads - 1) / kRapsdThreads), dim3(kRapsdThreads), 0, s, m, n, nb, shifted,
                     counts_dev);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

}  // namespace
}  // namespace psh

using psh::fail;

extern "C" int psh_rapsd_counts_dev(int m, int n, int shifted, unsigned long long *counts_dev) {
  using namespace psh;
  PSH_ENTER(c);
  if (!counts_dev) return fail(PSH_EINVAL, "rapsd_counts: NULL pointer");
  if (int rc = check_shape("rapsd_counts", 1, m, n)) return rc;
  return launch_count(m, n, shifted, counts_dev, c.stream);
}

extern "C" int psh_rapsd_half_dev(const void *spec_dev, int K, int m, int n, double *out_dev, unsigned long long *counts_dev) {
  using namespace psh;
  PSH_ENTER(c);
  if (!spec_dev || !out_dev || !counts_dev) return fail(PSH_EINVAL, "rapsd_half: NULL pointer");
  if (int rc = check_shape("rapsd_half", K, m, n)) return rc;
  if (reinterpret_cast<uintptr_t>(spec_dev) % 16) return fail(PSH_EINVAL, "rapsd_half: the spectra are not aligned to 16 bytes");
  const int nb = rapsd_bins(m, n), G = groups_for(m), bx = (nb + kRapsdThreads - 1) / kRapsdThreads;
  psh::Scratch blk;
  if (int rc = blk.alloc(static_cast<size_t>(K) * G * nb * sizeof(dd))) return rc;
  if (int rc = launch_count(m, n, 0, counts_dev, c.stream)) return rc;
  hipLaunchKernelGGL(rapsd_partial_half, dim3(bx, G, K), dim3(kRapsdThreads), 0, c.stream,
                     static_cast<const double2 *>(spec_dev), m, n, nb, blk.as<dd>());
  PSH_HIP(hipGetLastError());
  hipLaunchKernelGGL(rapsd_finish, dim3(bx, K), dim3(kRapsdThreads), 0, c.stream, blk.as<const dd>(), G, nb,
                     static_cast<const unsigned long long *>(counts_dev), static_cast<double>(m) * n, out_dev);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

extern "C" int psh_rapsd_full_dev(const void *planes_dev, int f64, int K, int m, int n, double *out_dev,
                                  unsigned long long *counts_dev) {
  using namespace psh;
  PSH_ENTER(c);
  if (!planes_dev || !out_dev || !counts_dev) return fail(PSH_EINVAL, "rapsd_full: NULL pointer");
  if (int rc = check_shape("rapsd_full", K, m, n)) return rc;
  if (reinterpret_cast<uintptr_t>(planes_dev) % (f64 ? 8 : 4)) return fail(PSH_EINVAL, "rapsd_full: the planes are not aligned to their element size");
  const int nb = rapsd_bins(m, n), G = groups_for(m), bx = (nb + kRapsdThreads - 1) / kRapsdThreads;
  psh::Scratch blk;
  if (int rc = blk.alloc(static_cast<size_t>(K) * G * nb * sizeof(dd))) return rc;
  if (int rc = launch_count(m, n, 1, counts_dev, c.stream)) return rc;
  with_real(planes_dev, f64 != 0, [&](auto *planes) {
    hipLaunchKernelGGL(rapsd_partial_full, dim3(bx, G, K), dim3(kRapsdThreads), 0, c.stream, planes, m, n, nb, blk.as<dd>());
  });
  PSH_HIP(hipGetLastError());
  hipLaunchKernelGGL(rapsd_finish, dim3(bx, K), dim3(kRapsdThreads), 0, c.stream, blk.as<const dd>(), G, nb,
                     static_cast<const unsigned long long *>(counts_dev), 1.0, out_dev);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

extern "C" int psh_rapsd_nonfinite_dev(const void *in_dev, int f64, size_t count, unsigned long long *counts_host) {
  using namespace psh;
  PSH_ENTER(c);
  if (!in_dev || !counts_host) return fail(PSH_EINVAL, "rapsd_nonfinite: NULL pointer");
  psh::Scratch blk;
  if (int rc = blk.alloc(2 * sizeof(unsigned long long))) return rc;
  unsigned long long *acc = blk.as<unsigned long long>();
  PSH_HIP(hipMemsetAsync(acc, 0, 2 * sizeof(unsigned long long), c.stream));
  if (count) {
    const size_t want = (count + kRapsdThreads - 1) / kRapsdThreads;
    const unsigned blocks = static_cast<unsigned>(want < 2048 ? want : 2048);
    with_real(in_dev, f64 != 0, [&](auto *in) {
      hipLaunchKernelGGL(rapsd_nonfinite, dim3(blocks), dim3(kRapsdThreads), 0, c.stream, in, count, acc);
    });
    PSH_HIP(hipGetLastError());
  }
  PSH_HIP(hipMemcpyAsync(counts_host, acc, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c.stream));
  PSH_HIP(hipStreamSynchronize(c.stream));
  return PSH_OK;
}

extern "C" int psh_rapsd_fill_nan_dev(const void *in_dev, int f64, size_t count, double fill, double *out_dev) {
  using namespace psh;
  PSH_ENTER(c);
  if (!in_dev || !out_dev) return fail(PSH_EINVAL, "rapsd_fill_nan: NULL pointer");
  if (!count) return PSH_OK;
  const size_t want = (count + kRapsdThreads - 1) / kRapsdThreads;
  const unsigned blocks = static_cast<unsigned>(want < 4096 ? want : 4096);
  with_real(in_dev, f64 != 0, [&](auto *in) {
    hipLaunchKernelGGL(rapsd_fill_nan, dim3(blocks), dim3(kRapsdThreads), 0, c.stream, in, count, fill, out_dev);
  });
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}
