// Temporal autocorrelation of a cascade on the device: the sums behind pysteps/timeseries/correlation.py
// (temporal_autocorrelation), every cascade level and every lag from one read of the stack.
//
//  * psh_autocorr_sums_dev           - spatial domain: per level, over the masked pixels, with a = x[-1] and
//                                      b_k = x[-(k+2)]: sum a, sum a^2 and per lag sum b_k, sum b_k^2, sum a b_k
//  * psh_autocorr_spectral_sums_dev  - spectral domain (pysteps/utils/spectral.py:62-76, corrcoef): per level
//                                      sum h |X|^2 and per lag Re sum h X conj(Y_k), sum h |Y_k|^2
//  * psh_autocorr_window_prepare_dev - the moving window's inputs: np.diff, x[~mask] = 0, mask.astype(float)
//  * psh_window_corrcoef_dev         - the element-wise finish of _moving_window_corrcoef (correlation.py:257-269)
//
// The sums are carried as double-double pairs (dd.h) with exact products, so the host can finish a coefficient in
// rational arithmetic and round once.  A thread owns a pixel for all planes of a level; every block writes its partial
// sums and one block per sum finishes them in a fixed order (no floating-point atomics; the counts are integer
// atomics, exact in any order).  Which pixels a thread adds, and in which order, depends on the pixel count alone:
// the same bits from run to run, for any number of levels and wherever a stack lies in memory.
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "dd.h"
#include "detsums.h"  // dd_add_prod

namespace psh {
namespace {

constexpr int kAcThreads = 256;
constexpr int kAcWaves = kAcThreads / 64;
constexpr int kAcPartBlocks = 512;  // partial sums per level at most - fixed: the summation order is part of the result
constexpr int kAcMaxLags = 8;

__device__ __forceinline__ double widen(double v) { return v; }
__device__ __forceinline__ double widen(float v) { return static_cast<double>(v); }

// the two pixels 2 p, 2 p + 1 of one plane.  VEC: one 16-byte (float: 8-byte) load - the plane starts on that boundary
// and has an even pixel count; otherwise element by element.  The values, and what is done with them, are the same.
template <bool VEC> __device__ __forceinline__ void load_pair(const double *plane, size_t p, size_t npix, double &v0, double &v1) {
  if (VEC) {
    const double2 t = reinterpret_cast<const double2 *>(plane)[p];
    v0 = t.x;
    v1 = t.y;
  } else {
    v0 = plane[2 * p];
    v1 = 2 * p + 1 < npix ? plane[2 * p + 1] : 0.0;
  }
}
template <bool VEC> __device__ __forceinline__ void load_pair(const float *plane, size_t p, size_t npix, double &v0, double &v1) {
  if (VEC) {
    const float2 t = reinterpret_cast<const float2 *>(plane)[p];
    v0 = widen(t.x);
    v1 = widen(t.y);
  } else {
    v0 = widen(plane[2 * p]);
    v1 = 2 * p + 1 < npix ? widen(plane[2 * p + 1]) : 0.0;
  }
}

__device__ __forceinline__ unsigned wave_sum_u32(unsigned c) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d);
  return c;
}

// the block's sums into partial[(blockIdx.y * gridDim.x + blockIdx.x) * nsums + s]
template <int NMAX> __device__ __forceinline__ void block_store(const dd (&acc)[NMAX], int nsums, dd *__restrict__ partial) {
  __shared__ dd s_part[kAcWaves][NMAX];
#pragma unroll
  for (int s = 0; s < NMAX; ++s) {
    if (s < nsums) {
      const dd t = dd_wave_sum(acc[s]);
      if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6][s] = t;
    }
  }
  __syncthreads();
  if (static_cast<int>(threadIdx.x) < nsums) {
    dd t = s_part[0][threadIdx.x];
    for (int w = 1; w < kAcWaves; ++w) t = dd_add(t, s_part[w][threadIdx.x]);
    partial[(static_cast<size_t>(blockIdx.y) * gridDim.x + blockIdx.x) * nsums + threadIdx.x] = t;
  }
}

// grid (blocks, levels).  KMAX: the lags the registers are laid out for (K <= KMAX is the call's).  The planes are
// indexed from the newest: w[j] = x[-(j+1)], so that a and b_k sit at fixed registers whatever the series' length.
template <class T, int KMAX, bool VEC>
__global__ __launch_bounds__(kAcThreads) void autocorr_partial(const T *__restrict__ x, int nframes, int d, size_t npix,
                                                              const unsigned char *__restrict__ mask, dd *__restrict__ partial,
                                                              unsigned long long *__restrict__ count,
                                                              unsigned long long *__restrict__ nonfinite) {
#pragma clang fp contract(off)
  constexpr int NMAX = 2 + 3 * KMAX;
  const int K = nframes - d - 1;
  const T *level = x + static_cast<size_t>(blockIdx.y) * nframes * npix;
  dd acc[NMAX];
#pragma unroll
  for (int s = 0; s < NMAX; ++s) acc[s] = {0.0, 0.0};
  unsigned n_masked = 0, n_bad = 0;
  const size_t npairs = (npix + 1) / 2;
  const size_t stride = static_cast<size_t>(gridDim.x) * kAcThreads;
  for (size_t p = static_cast<size_t>(blockIdx.x) * kAcThreads + threadIdx.x; p < npairs; p += stride) {
    double w[KMAX + 2][2];
#pragma unroll
    for (int j = 0; j < KMAX + 2; ++j) {
      if (j < nframes) load_pair<VEC>(level + static_cast<size_t>(nframes - 1 - j) * npix, p, npix, w[j][0], w[j][1]);
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const size_t i = 2 * p + e;
      if (i >= npix) break;
#pragma unroll
      for (int j = 0; j < KMAX + 2; ++j) {
        if (j < nframes && !isfinite(w[j][e])) ++n_bad;
      }
      if (mask && !mask[i]) continue;
      ++n_masked;
      double s[KMAX + 1];  // the (differenced) series, newest first
#pragma unroll
      for (int j = 0; j < KMAX + 1; ++j) {
        if (j <= K) s[j] = d ? w[j][e] - w[j + 1][e] : w[j][e];
      }
      const double a = s[0];
      acc[0] = dd_add_d(acc[0], a);
      acc[1] = dd_add_sq(acc[1], a);
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        if (k < K) {
          const double b = s[k + 1];
          acc[2 + 3 * k] = dd_add_d(acc[2 + 3 * k], b);
          acc[3 + 3 * k] = dd_add_sq(acc[3 + 3 * k], b);
          acc[4 + 3 * k] = dd_add_prod(acc[4 + 3 * k], a, b);
        }
      }
    }
  }
  block_store<NMAX>(acc, 2 + 3 * K, partial);
  n_masked = wave_sum_u32(n_masked);
  n_bad = wave_sum_u32(n_bad);
  if ((threadIdx.x & 63) == 0) {
    if (blockIdx.y == 0 && n_masked) atomicAdd(count, static_cast<unsigned long long>(n_masked));
    if (n_bad) atomicAdd(nonfinite + blockIdx.y, static_cast<unsigned long long>(n_bad));
  }
}

__device__ __forceinline__ double herm(size_t col, int nc, int n_even, int full) {
  return (full || col == 0 || (n_even && col == static_cast<size_t>(nc) - 1)) ? 1.0 : 2.0;
}

// spectra (levels, nframes, m, nc) complex128; grid (blocks, levels); sums per level: [0] = sum h |X|^2,
// [1 + 2 k] = Re sum h X conj(Y_k), [2 + 2 k] = sum h |Y_k|^2
template <int KMAX>
__global__ __launch_bounds__(kAcThreads) void autocorr_spectral_partial(const double2 *__restrict__ x, int nframes, int d, size_t plane,
                                                                       int nc, int n_even, int full, dd *__restrict__ partial,
                                                                       unsigned long long *__restrict__ nonfinite) {
#pragma clang fp contract(off)
  constexpr int NMAX = 1 + 2 * KMAX;
  const int K = nframes - d - 1;
  const double2 *level = x + static_cast<size_t>(blockIdx.y) * nframes * plane;
  dd acc[NMAX];
#pragma unroll
  for (int s = 0; s < NMAX; ++s) acc[s] = {0.0, 0.0};
  unsigned n_bad = 0;
  const size_t stride = static_cast<size_t>(gridDim.x) * kAcThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kAcThreads + threadIdx.x; i < plane; i += stride) {
    double2 w[KMAX + 2];
#pragma unroll
    for (int j = 0; j < KMAX + 2; ++j) {
      if (j < nframes) {
        w[j] = level[static_cast<size_t>(nframes - 1 - j) * plane + i];
        if (!isfinite(w[j].x) || !isfinite(w[j].y)) ++n_bad;
      }
    }
    const double h = herm(i % static_cast<size_t>(nc), nc, n_even, full);
    double2 s[KMAX + 1];
#pragma unroll
    for (int j = 0; j < KMAX + 1; ++j) {
      if (j <= K) s[j] = d ? make_double2(w[j].x - w[j + 1].x, w[j].y - w[j + 1].y) : w[j];
    }
    // h is 1 or 2: h * v is exact, and so is every product below
    const double ar = s[0].x, ai = s[0].y, har = h * s[0].x, hai = h * s[0].y;
    acc[0] = dd_add_prod(acc[0], har, ar);
    acc[0] = dd_add_prod(acc[0], hai, ai);
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      if (k < K) {
        const double br = s[k + 1].x, bi = s[k + 1].y;
        acc[1 + 2 * k] = dd_add_prod(acc[1 + 2 * k], har, br);
        acc[1 + 2 * k] = dd_add_prod(acc[1 + 2 * k], hai, bi);
        acc[2 + 2 * k] = dd_add_prod(acc[2 + 2 * k], h * br, br);
        acc[2 + 2 * k] = dd_add_prod(acc[2 + 2 * k], h * bi, bi);
      }
    }
  }
  block_store<NMAX>(acc, 1 + 2 * K, partial);
  n_bad = wave_sum_u32(n_bad);
  if ((threadIdx.x & 63) == 0 && n_bad) atomicAdd(nonfinite + blockIdx.y, static_cast<unsigned long long>(n_bad));
}

// sums[level][s] = the level's partial sums of s in block order; grid (nsums, levels)
__global__ __launch_bounds__(kAcThreads) void autocorr_final(const dd *__restrict__ partial, int nblocks, int nsums, dd *__restrict__ sums) {
  __shared__ dd s_part[kAcWaves];
  const dd *src = partial + static_cast<size_t>(blockIdx.y) * nblocks * nsums + blockIdx.x;
  dd acc = {0.0, 0.0};
  for (int i = threadIdx.x; i < nblocks; i += kAcThreads) acc = dd_add(acc, src[static_cast<size_t>(i) * nsums]);
  acc = dd_wave_sum(acc);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    dd t = s_part[0];
    for (int w = 1; w < kAcWaves; ++w) t = dd_add(t, s_part[w]);
    sums[static_cast<size_t>(blockIdx.y) * nsums + blockIdx.x] = t;
  }
}

// out (1 + nframes - d, npix): out[0] = mask.astype(float); out[1 + j] = the (differenced) plane j, in time order,
// with x[~mask] = 0.0 (correlation.py:232-236).  nonfinite: over every pixel of every input plane
__global__ __launch_bounds__(kAcThreads) void window_prepare(const double *__restrict__ x, int nframes, int d, size_t npix,
                                                            const unsigned char *__restrict__ mask, double *__restrict__ out,
                                                            unsigned long long *__restrict__ nonfinite) {
#pragma clang fp contract(off)
  unsigned n_bad = 0;
  const size_t stride = static_cast<size_t>(gridDim.x) * kAcThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kAcThreads + threadIdx.x; i < npix; i += stride) {
    const bool in = !mask || mask[i];
    out[i] = in ? 1.0 : 0.0;
    double prev = x[i];
    if (!isfinite(prev)) ++n_bad;
    if (!d) out[npix + i] = in ? prev : 0.0;
    for (int t = 1; t < nframes; ++t) {
      const double v = x[static_cast<size_t>(t) * npix + i];
      if (!isfinite(v)) ++n_bad;
      out[static_cast<size_t>(1 + t - d) * npix + i] = in ? (d ? v - prev : v) : 0.0;
      prev = v;
    }
  }
  n_bad = wave_sum_u32(n_bad);
  if ((threadIdx.x & 63) == 0 && n_bad) atomicAdd(nonfinite, static_cast<unsigned long long>(n_bad));
}

// correlation.py:248-269, one array operation of the reference per line, each rounded on its own
__global__ __launch_bounds__(kAcThreads) void window_corrcoef(const double *__restrict__ fn, const double *__restrict__ fsx,
                                                             const double *__restrict__ fsy, const double *__restrict__ fssx,
                                                             const double *__restrict__ fssy, const double *__restrict__ fsxy,
                                                             double factor, size_t count, double *__restrict__ out) {
#pragma clang fp contract(off)
  const size_t stride = static_cast<size_t>(gridDim.x) * kAcThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kAcThreads + threadIdx.x; i < count; i += stride) {
    const double n = fn[i] * factor;  // convol_filter(...) * window_size**2
    const double sx = fsx[i] * factor;
    const double sy = fsy[i] * factor;
    const double ssx = fssx[i] * factor;
    const double ssy = fssy[i] * factor;
    const double sxy = fsxy[i] * factor;
    const double mux = sx / n;
    const double muy = sy / n;
    const double tx = 2.0 * mux;
    const double ty = 2.0 * muy;
    const double varx = (ssx - tx * sx) + n * (mux * mux);  // ssx - 2 * mux * sx + n * mux**2
    const double vary = (ssy - ty * sy) + n * (muy * muy);
    const double stdx = sqrt(varx);
    const double stdy = sqrt(vary);
    const double nmux = n * mux;
    const double cov = ((sxy - muy * sx) - mux * sy) + nmux * muy;  // sxy - muy * sx - mux * sy + n * mux * muy
    const double sxsy = stdx * stdy;
    const bool ok = stdx > 1e-8 && stdy > 1e-8 && sxsy > 1e-8 && n >= 3.0;
    out[i] = ok ? cov / sxsy : NAN;
  }
}

unsigned ac_blocks(size_t items) {
  const size_t blocks = (items + kAcThreads - 1) / kAcThreads;
  return static_cast<unsigned>(blocks < static_cast<size_t>(kAcPartBlocks) ? (blocks ? blocks : 1) : kAcPartBlocks);
}

template <class T, int KMAX>
void launch_partial(bool vec, dim3 grid, hipStream_t stream, const T *x, int nframes, int d, size_t npix, const unsigned char *mask,
                    dd *partial, unsigned long long *count, unsigned long long *nonfinite) {
  if (vec)
    hipLaunchKernelGGL((autocorr_partial<T, KMAX, true>), grid, dim3(kAcThreads), 0, stream, x, nframes, d, npix, mask, partial, count,
                       nonfinite);
  else
    hipLaunchKernelGGL((autocorr_partial<T, KMAX, false>), grid, dim3(kAcThreads), 0, stream, x, nframes, d, npix, mask, partial, count,
                       nonfinite);
}

}  // namespace
}  // namespace psh

using psh::fail;

extern "C" int psh_autocorr_sums_dev(const void *stack_dev, int is_f64, int nlevels, int nframes, size_t npix,
                                     const unsigned char *mask_dev, int d, double *sums_dev, unsigned long long *count_dev,
                                     unsigned long long *nonfinite_dev) {
  PSH_ENTER(c);
  if (!stack_dev || !sums_dev || !count_dev || !nonfinite_dev) return fail(PSH_EINVAL, "autocorr_sums: NULL pointer");
  if (d != 0 && d != 1) return fail(PSH_EINVAL, "autocorr_sums: d must be 0 or 1");
  if (nlevels < 1 || nlevels > 65535 || npix == 0) return fail(PSH_EINVAL, "autocorr_sums: 1..65535 levels, not empty");
  const int K = nframes - d - 1;
  if (K < 1) return fail(PSH_EINVAL, "autocorr_sums: at least %d frames", 2 + d);
  if (K > psh::kAcMaxLags) return fail(PSH_EUNSUPPORTED, "autocorr_sums: at most %d lags", psh::kAcMaxLags);
  const size_t item = is_f64 ? sizeof(double) : sizeof(float);
  if (reinterpret_cast<uintptr_t>(stack_dev) % item) return fail(PSH_EINVAL, "autocorr_sums: misaligned stack");
  const int nsums = 2 + 3 * K;
  const unsigned blocks = psh::ac_blocks((npix + 1) / 2);
  psh::Scratch partial;
  if (int rc = partial.alloc(static_cast<size_t>(nlevels) * blocks * nsums * sizeof(psh::dd))) return rc;
  PSH_HIP(hipMemsetAsync(count_dev, 0, sizeof(unsigned long long), c.stream));
  PSH_HIP(hipMemsetAsync(nonfinite_dev, 0, static_cast<size_t>(nlevels) * sizeof(unsigned long long), c.stream));
  // every plane starts on a two-element boundary: the stack does and the planes hold an even number of pixels
  const bool vec = npix % 2 == 0 && reinterpret_cast<uintptr_t>(stack_dev) % (2 * item) == 0;
  const dim3 grid(blocks, nlevels);
  psh::dd *part = partial.as<psh::dd>();
  psh::with_real(stack_dev, is_f64 != 0, [&](auto *x) {
    using T = std::remove_cv_t<std::remove_pointer_t<decltype(x)>>;
    if (K <= 2)
      psh::launch_partial<T, 2>(vec, grid, c.stream, x, nframes, d, npix, mask_dev, part, count_dev, nonfinite_dev);
    else
      psh::launch_partial<T, psh::kAcMaxLags>(vec, grid, c.stream, x, nframes, d, npix, mask_dev, part, count_dev, nonfinite_dev);
    return 0;
  });
  PSH_HIP(hipGetLastError());
  hipLaunchKernelGGL(psh::autocorr_final, dim3(nsums, nlevels), dim3(psh::kAcThreads), 0, c.stream, static_cast<const psh::dd *>(part),
                     static_cast<int>(blocks), nsums, reinterpret_cast<psh::dd *>(sums_dev));
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

extern "C" int psh_autocorr_spectral_sums_dev(const void *spec_dev, int nlevels, int nframes, int m, int nc, int n, int full_fft,
                                              int d, double *sums_dev, unsigned long long *nonfinite_dev) {
  PSH_ENTER(c);
  if (!spec_dev || !sums_dev || !nonfinite_dev) return fail(PSH_EINVAL, "autocorr_spectral_sums: NULL pointer");
  if (d != 0 && d != 1) return fail(PSH_EINVAL, "autocorr_spectral_sums: d must be 0 or 1");
  if (nlevels < 1 || nlevels > 65535 || m < 1 || n < 1) return fail(PSH_EINVAL, "autocorr_spectral_sums: invalid shape");
  if (nc != (full_fft ? n : n / 2 + 1)) return fail(PSH_EINVAL, "autocorr_spectral_sums: %d columns do not belong to a width of %d", nc, n);
  const int K = nframes - d - 1;
  if (K < 1) return fail(PSH_EINVAL, "autocorr_spectral_sums: at least %d frames", 2 + d);
  if (K > psh::kAcMaxLags) return fail(PSH_EUNSUPPORTED, "autocorr_spectral_sums: at most %d lags", psh::kAcMaxLags);
  if (reinterpret_cast<uintptr_t>(spec_dev) % sizeof(double2)) return fail(PSH_EINVAL, "autocorr_spectral_sums: misaligned spectra");
  const int nsums = 1 + 2 * K;
  const size_t plane = static_cast<size_t>(m) * nc;
  const unsigned blocks = psh::ac_blocks(plane);
  psh::Scratch partial;
  if (int rc = partial.alloc(static_cast<size_t>(nlevels) * blocks * nsums * sizeof(psh::dd))) return rc;
  PSH_HIP(hipMemsetAsync(nonfinite_dev, 0, static_cast<size_t>(nlevels) * sizeof(unsigned long long), c.stream));
  psh::dd *part = partial.as<psh::dd>();
  const double2 *x = static_cast<const double2 *>(spec_dev);
  const int n_even = (n & 1) == 0 ? 1 : 0;
  if (K <= 2)
    hipLaunchKernelGGL(psh::autocorr_spectral_partial<2>, dim3(blocks, nlevels), dim3(psh::kAcThreads), 0, c.stream, x, nframes, d, plane, nc,
                       n_even, full_fft ? 1 : 0, part, nonfinite_dev);
  else
    hipLaunchKernelGGL(psh::autocorr_spectral_partial<psh::kAcMaxLags>, dim3(blocks, nlevels), dim3(psh::kAcThreads), 0, c.stream, x, nframes,
                       d, plane, nc, n_even, full_fft ? 1 : 0, part, nonfinite_dev);
  PSH_HIP(hipGetLastError());
  hipLaunchKernelGGL(psh::autocorr_final, dim3(nsums, nlevels), dim3(psh::kAcThreads), 0, c.stream, static_cast<const psh::dd *>(part),
                     static_cast<int>(blocks), nsums, reinterpret_cast<psh::dd *>(sums_dev));
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

extern "C" int psh_autocorr_window_prepare_dev(const double *stack_dev, int nframes, size_t npix, const unsigned char *mask_dev, int d,
                                               double *out_dev, unsigned long long *nonfinite_dev) {
  PSH_ENTER(c);
  if (!stack_dev || !out_dev || !nonfinite_dev) return fail(PSH_EINVAL, "autocorr_window_prepare: NULL pointer");
  if ((d != 0 && d != 1) || nframes - d < 2 || npix == 0) return fail(PSH_EINVAL, "autocorr_window_prepare: d 0 or 1, two planes after it");
  PSH_HIP(hipMemsetAsync(nonfinite_dev, 0, sizeof(unsigned long long), c.stream));
  hipLaunchKernelGGL(psh::window_prepare, dim3(static_cast<unsigned>(std::min<size_t>((npix + psh::kAcThreads - 1) / psh::kAcThreads, 4096))), dim3(psh::kAcThreads), 0,
                     c.stream, stack_dev, nframes, d, npix, mask_dev, out_dev, nonfinite_dev);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

extern "C" int psh_window_corrcoef_dev(const double *n_dev, const double *sx_dev, const double *sy_dev, const double *ssx_dev,
                                       const double *ssy_dev, const double *sxy_dev, double factor, size_t count, double *out_dev) {
  PSH_ENTER(c);
  if (!n_dev || !sx_dev || !sy_dev || !ssx_dev || !ssy_dev || !sxy_dev || !out_dev) return fail(PSH_EINVAL, "window_corrcoef: NULL pointer");
  if (count == 0) return fail(PSH_EINVAL, "window_corrcoef: empty planes");
  hipLaunchKernelGGL(psh::window_corrcoef, dim3(static_cast<unsigned>(std::min<size_t>((count + psh::kAcThreads - 1) / psh::kAcThreads, 4096))), dim3(psh::kAcThreads),
                     0, c.stream, n_dev, sx_dev, sy_dev, ssx_dev, ssy_dev, sxy_dev, factor, count, out_dev);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}
