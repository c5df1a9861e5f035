// The noise standard-deviation adjustment of STEPS on the device: what pysteps/noise/utils.py:24-135
// (compute_noise_stddev_adjs) does per noise realisation between the noise filter and the cascade decomposition
// (cascade.hip), and the level statistics it compares.  float64 throughout like the reference; every reduction
// writes block partial sums that one block finishes in a fixed order (no floating-point atomics), so the results do
// not change from run to run or with the number of realisations handed over at once.
//
//  * psh_noise_adj_observed_dev      - utils.py:83-87: MASK = R >= R_thr_1, R[~isfinite(R)] = R[~MASK] = R_thr_2
//  * psh_noise_adj_centre_dev        - utils.py:92: R -= mu
//  * psh_noise_adj_prepare_dev       - utils.py:113-118 on a batch of filtered noise fields
//  * psh_mask_count_dev              - number of set bytes of a mask
//  * psh_masked_moments_dev          - np.mean(x[mask]), np.std(x[mask]) of cascade/decomposition.py:223-228
//  * psh_spectrum_level_moments_dev  - the unmasked level statistics read off the field's half spectrum
//  * psh::moments                    - np.mean(x), np.std(x) of whole planes for cascade.hip and the prepare stage
#include <algorithm>

#include "common.h"
#include "dd.h"

namespace psh {
namespace {

constexpr int kThreads = 256;
constexpr int kPartBlocks = 512;  // partial sums per plane (moments) - fixed: the summation order is part of the result
constexpr int kMaxLevels = 16;

// ---- double-double accumulation ---------------------------------------------------------------------------
// The masked moments are taken with a shift of ZERO (a shift picked from the data - the first wet pixel - would
// need a scan of the mask before the sums could start, and would tie the rounding to where that pixel lies).  A
// zero shift leaves var = E[x^2] - E[x]^2 to cancel wherever a level's mean over the wet pixels is not small
// beside its spread (level 0 carries the masked field's mean), so the two sums are carried as unevaluated pairs
// hi + lo (Knuth's two-sum, the product's error from an fma): ~106 bits, the cancellation then costs nothing
// that shows in a double, and the order of the additions stops mattering at the 1e-16 level.  The kernel is
// bound by the planes' bytes, the extra flops are free.  The helpers are in dd.h.
// The moments of whole planes (psh::moments below) are the same kernels without a mask.  They used to be plain
// double sums of x - x[0]: fine while x[0] lies within a few standard deviations of the mean, but with
// d = |x[0] - mean| / std the subtraction E[v^2] - E[v]^2 loses about d^2 of the significand (a rain cell on the
// field's first pixel: d ~ sqrt(pixels)), and x - x[0] is itself rounded, so no shift taken from the data is exact.

// one block's {sum, sum of squares} of a plane as four doubles
struct Part {
  dd s, q;
};

__device__ __forceinline__ Part block_sum(Part v, Part *s_part) {  // valid in thread 0
  v.s = dd_wave_sum(v.s);
  v.q = dd_wave_sum(v.q);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
  __syncthreads();
  Part t = s_part[0];
  if (threadIdx.x == 0) {
    for (int w = 1; w < kThreads / 64; ++w) {
      t.s = dd_add(t.s, s_part[w].s);
      t.q = dd_add(t.q, s_part[w].q);
    }
  }
  __syncthreads();
  return t;
}

// P consecutive planes per block (blockIdx.y * P ...): the mask byte of a pixel is read once for the P planes.
// The pixels a thread adds and their order do not depend on P, so every P gives the same bits.  Measured on the
// MI355X at 4096^2 with 8 planes (tools/noise_adj_quick.py): P = 1 0.239 ms, P = 4 0.262 ms - sharing the byte does
// not pay, the Python layer asks for P = 1.
template <int P>
__global__ __launch_bounds__(kThreads) void masked_partial(const double *__restrict__ x, int nplanes, size_t plane,
                                                           const unsigned char *__restrict__ mask, Part *__restrict__ partial) {
  __shared__ Part s_part[kThreads / 64];
  const int p0 = blockIdx.y * P;
  Part acc[P];
#pragma unroll
  for (int j = 0; j < P; ++j) acc[j] = {{0.0, 0.0}, {0.0, 0.0}};
  const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < plane; i += stride) {
    if (mask && !mask[i]) continue;  // no mask: every pixel (psh::moments)
#pragma unroll
    for (int j = 0; j < P; ++j) {
      if (p0 + j < nplanes) {
        const double v = x[static_cast<size_t>(p0 + j) * plane + i];
        acc[j].s = dd_add_d(acc[j].s, v);
        acc[j].q = dd_add_sq(acc[j].q, v);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const Part t = block_sum(acc[j], s_part);
    if (threadIdx.x == 0 && p0 + j < nplanes) partial[static_cast<size_t>(p0 + j) * gridDim.x + blockIdx.x] = t;
  }
}

// stats[p] = {mean, population std} over `*count` pixels (count == nullptr: over `pixels`, the whole plane); one block
// per plane.  A NaN in the plane leaves NaN in both (an infinity too: Inf - Inf in the two-sums), like np.std.
__global__ __launch_bounds__(kThreads) void masked_final(const Part *__restrict__ partial, int nblocks,
                                                         const unsigned long long *__restrict__ count,
                                                         unsigned long long pixels, double2 *__restrict__ stats) {
  __shared__ Part s_part[kThreads / 64];
  const Part *src = partial + static_cast<size_t>(blockIdx.x) * nblocks;
  Part acc = {{0.0, 0.0}, {0.0, 0.0}};
  for (int i = threadIdx.x; i < nblocks; i += kThreads) {
    acc.s = dd_add(acc.s, src[i].s);
    acc.q = dd_add(acc.q, src[i].q);
  }
  const Part t = block_sum(acc, s_part);
  if (threadIdx.x == 0) {
    const double cnt = static_cast<double>(count ? *count : pixels);  // 0: 0 / 0 = NaN, like NumPy on an empty selection
    const dd mean = dd_div_d(t.s, cnt);
    const dd m2 = dd_sqr(mean);
    const dd ex2 = dd_div_d(t.q, cnt);
    const dd var = dd_add(ex2, {-m2.hi, -m2.lo});
    const double v = var.hi + var.lo;
    stats[blockIdx.x] = make_double2(mean.hi + mean.lo, v > 0.0 ? sqrt(v) : (v == v ? 0.0 : v));
  }
}

// integer count of the set bytes (integer atomics: exact in any order)
__global__ __launch_bounds__(kThreads) void mask_count(const unsigned char *__restrict__ mask, size_t plane,
                                                       unsigned long long *__restrict__ count) {
  unsigned c = 0;
  const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < plane; i += stride) c += mask[i] ? 1u : 0u;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, static_cast<unsigned long long>(c));
}

// utils.py:83-87
__global__ __launch_bounds__(kThreads) void observed(const double *__restrict__ r, size_t plane, double thr1, double thr2,
                                                     unsigned char *__restrict__ mask, double *__restrict__ clean) {
  const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < plane; i += stride) {
    const double v = r[i];
    const bool wet = v >= thr1;  // NaN: false
    mask[i] = wet ? 1 : 0;
    clean[i] = (wet && isfinite(v)) ? v : thr2;
  }
}

__global__ __launch_bounds__(kThreads) void centre(double *__restrict__ x, size_t n, double mu) {
  const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) x[i] = x[i] - mu;
}

// utils.py:113-118, one array operation of the reference per line (each rounded on its own); blockIdx.y = realisation
__global__ __launch_bounds__(kThreads) void prepare(double *__restrict__ fields, size_t plane,
                                                    const unsigned char *__restrict__ mask,
                                                    const double2 *__restrict__ stats, double sigma, double mu, double thr2) {
#pragma clang fp contract(off)
  double *x = fields + static_cast<size_t>(blockIdx.y) * plane;
  const double sd = stats[blockIdx.y].y;
  const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < plane; i += stride) {
    const double a = x[i] / sd;   // N / np.std(N)
    const double b = a * sigma;   // * sigma
    double c = b + mu;            // + mu
    if (!mask[i]) c = thr2;       // N[~MASK] = R_thr_2
    x[i] = c - mu;                // N -= mu
  }
}

__device__ __forceinline__ double herm_weight(int c, int nc, int n_even) { return (c == 0 || (n_even && c == nc - 1)) ? 1.0 : 2.0; }

// partial[spec][block][k] = sum over the block's rows of herm |X W_k|^2, the DC coefficient left out (it is the level's
// mean, which np.std removes); blockIdx.y = spectrum.  The spectrum is read once for all levels.
__global__ __launch_bounds__(kThreads) void spectrum_partial(const double2 *__restrict__ spec, const double *__restrict__ weights,
                                                             int nlevels, int m, int nc, int n_even, double *__restrict__ partial) {
  __shared__ double s_part[kThreads / 64][kMaxLevels];
  const size_t plane = static_cast<size_t>(m) * nc;
  const double2 *x = spec + static_cast<size_t>(blockIdx.y) * plane;
  double acc[kMaxLevels];
#pragma unroll
  for (int k = 0; k < kMaxLevels; ++k) acc[k] = 0.0;
  for (int r = blockIdx.x; r < m; r += gridDim.x) {  // whole rows per block: the column's weight without a division
    for (int c = threadIdx.x; c < nc; c += kThreads) {
      if (r == 0 && c == 0) continue;
      const size_t i = static_cast<size_t>(r) * nc + c;
      const double2 y = x[i];
      const double e = herm_weight(c, nc, n_even) * (y.x * y.x + y.y * y.y);
#pragma unroll
      for (int k = 0; k < kMaxLevels; ++k) {
        if (k < nlevels) {
          const double w = weights[static_cast<size_t>(k) * plane + i];
          acc[k] += e * (w * w);
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kMaxLevels; ++k) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc[k] += __shfl_xor(acc[k], d);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < kMaxLevels; ++k) s_part[threadIdx.x >> 6][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < kMaxLevels) {
    double t = 0.0;
    for (int w = 0; w < kThreads / 64; ++w) t += s_part[w][threadIdx.x];
    partial[(static_cast<size_t>(blockIdx.y) * gridDim.x + blockIdx.x) * kMaxLevels + threadIdx.x] = t;
  }
}

// stats[spec][k] = {X[0,0] W_k[0,0] / (m n), sqrt(sum) / (m n)}; grid (nlevels, nspec)
__global__ __launch_bounds__(kThreads) void spectrum_final(const double *__restrict__ partial, int nparts,
                                                           const double2 *__restrict__ spec, const double *__restrict__ weights,
                                                           size_t plane, double cells, double2 *__restrict__ stats) {
  __shared__ double s_part[kThreads / 64];
  const int k = blockIdx.x;
  const double *src = partial + static_cast<size_t>(blockIdx.y) * nparts * kMaxLevels;
  double t = 0.0;
  for (int i = threadIdx.x; i < nparts; i += kThreads) t += src[static_cast<size_t>(i) * kMaxLevels + k];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) t += __shfl_xor(t, d);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    double all = 0.0;
    for (int w = 0; w < kThreads / 64; ++w) all += s_part[w];
    const double dc = spec[static_cast<size_t>(blockIdx.y) * plane].x * weights[static_cast<size_t>(k) * plane];
    stats[static_cast<size_t>(blockIdx.y) * gridDim.x + k] = make_double2(dc / cells, sqrt(all) / cells);
  }
}

unsigned sweep_blocks(size_t n) {
  const size_t blocks = (n + kThreads - 1) / kThreads;
  return static_cast<unsigned>(blocks < 4096 ? (blocks ? blocks : 1) : 4096);
}

}  // namespace

// {mean, population std} of `planes` whole planes (declared in common.h; cascade.hip takes the level statistics, the
// field mean and the noise filter's standardisation from it, psh_noise_adj_prepare_dev np.std(N)): the masked kernels
// without a mask and with the plane's size for the count - one reduction, the same double-double sums in the same
// fixed order.  A plane's pair depends on its own values alone, not on where in the plane they lie beyond rounding at
// the 1e-16 level, nor on its neighbours or the number of planes.
int moments(const double *x_dev, int planes, size_t plane, double2 *stats_dev, hipStream_t stream) {
  Scratch partial;
  if (int rc = partial.alloc(static_cast<size_t>(planes) * kPartBlocks * sizeof(Part))) return rc;
  hipLaunchKernelGGL(masked_partial<1>, dim3(kPartBlocks, planes), dim3(kThreads), 0, stream, x_dev, planes, plane,
                     static_cast<const unsigned char *>(nullptr), partial.as<Part>());
  hipLaunchKernelGGL(masked_final, dim3(planes), dim3(kThreads), 0, stream, partial.as<const Part>(), kPartBlocks,
                     static_cast<const unsigned long long *>(nullptr), static_cast<unsigned long long>(plane), stats_dev);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

}  // namespace psh

using psh::fail;

extern "C" int psh_noise_adj_observed_dev(const double *r_dev, size_t plane, double thr1, double thr2,
                                          unsigned char *mask_dev, double *clean_dev) {
  PSH_ENTER(c);
  if (!r_dev || !mask_dev || !clean_dev) return fail(PSH_EINVAL, "noise_adj_observed: NULL pointer");
  if (plane == 0) return fail(PSH_EINVAL, "noise_adj_observed: empty field");
  hipLaunchKernelGGL(psh::observed, dim3(psh::sweep_blocks(plane)), dim3(psh::kThreads), 0, c.stream, r_dev, plane, thr1, thr2,
                     mask_dev, clean_dev);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

extern "C" int psh_noise_adj_centre_dev(double *field_dev, size_t n, double mu) {
  PSH_ENTER(c);
  if (!field_dev || n == 0) return fail(PSH_EINVAL, "noise_adj_centre: NULL pointer or empty field");
  hipLaunchKernelGGL(psh::centre, dim3(psh::sweep_blocks(n)), dim3(psh::kThreads), 0, c.stream, field_dev, n, mu);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

extern "C" int psh_noise_adj_prepare_dev(double *fields_dev, int nbatch, size_t plane, const unsigned char *mask_dev,
                                         double sigma, double mu, double thr2, double *stats_out_dev) {
  PSH_ENTER(c);
  if (!fields_dev || !mask_dev) return fail(PSH_EINVAL, "noise_adj_prepare: NULL pointer");
  if (nbatch < 1 || nbatch > 65535 || plane == 0) return fail(PSH_EINVAL, "noise_adj_prepare: 1..65535 fields, not empty");
  psh::Scratch stats;
  if (int rc = stats.alloc(static_cast<size_t>(nbatch) * sizeof(double2))) return rc;
  // np.std(N) of every realisation: the reduction the noise filter standardises with, per plane
  if (int rc = psh::moments(fields_dev, nbatch, plane, stats.as<double2>(), c.stream)) return rc;
  if (stats_out_dev)
    PSH_HIP(hipMemcpyAsync(stats_out_dev, stats.as<void>(), static_cast<size_t>(nbatch) * sizeof(double2), hipMemcpyDeviceToDevice, c.stream));
  hipLaunchKernelGGL(psh::prepare, dim3(std::min(psh::sweep_blocks(plane), 2048u), nbatch), dim3(psh::kThreads), 0, c.stream,
                     fields_dev, plane, mask_dev, stats.as<const double2>(), sigma, mu, thr2);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

extern "C" int psh_mask_count_dev(const unsigned char *mask_dev, size_t plane, unsigned long long *count_dev) {
  PSH_ENTER(c);
  if (!mask_dev || !count_dev) return fail(PSH_EINVAL, "mask_count: NULL pointer");
  PSH_HIP(hipMemsetAsync(count_dev, 0, sizeof(unsigned long long), c.stream));
  if (plane) hipLaunchKernelGGL(psh::mask_count, dim3(std::min(psh::sweep_blocks(plane), 1024u)), dim3(psh::kThreads), 0, c.stream,
                                mask_dev, plane, count_dev);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

extern "C" int psh_masked_moments_dev(const double *planes_dev, int nplanes, size_t plane, const unsigned char *mask_dev,
                                      const unsigned long long *count_dev, int planes_per_block, double *stats_dev) {
  PSH_ENTER(c);
  if (!planes_dev || !mask_dev || !count_dev || !stats_dev) return fail(PSH_EINVAL, "masked_moments: NULL pointer");
  if (nplanes < 1 || nplanes > 65535 || plane == 0) return fail(PSH_EINVAL, "masked_moments: 1..65535 planes, not empty");
  if (planes_per_block != 1 && planes_per_block != 4) return fail(PSH_EINVAL, "masked_moments: 1 or 4 planes per block");
  psh::Scratch partial;
  if (int rc = partial.alloc(static_cast<size_t>(nplanes) * psh::kPartBlocks * sizeof(psh::Part))) return rc;
  psh::Part *part = partial.as<psh::Part>();
  if (planes_per_block == 4)
    hipLaunchKernelGGL(psh::masked_partial<4>, dim3(psh::kPartBlocks, (nplanes + 3) / 4), dim3(psh::kThreads), 0, c.stream,
                       planes_dev, nplanes, plane, mask_dev, part);
  else
    hipLaunchKernelGGL(psh::masked_partial<1>, dim3(psh::kPartBlocks, nplanes), dim3(psh::kThreads), 0, c.stream, planes_dev,
                       nplanes, plane, mask_dev, part);
  hipLaunchKernelGGL(psh::masked_final, dim3(nplanes), dim3(psh::kThreads), 0, c.stream, static_cast<const psh::Part *>(part),
                     psh::kPartBlocks, count_dev, 0ull, reinterpret_cast<double2 *>(stats_dev));
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

extern "C" int psh_spectrum_level_moments_dev(const void *spec_dev, int nspec, const double *weights_dev, int nlevels, int m,
                                              int n, double *stats_dev) {
  PSH_ENTER(c);
  if (!spec_dev || !weights_dev || !stats_dev) return fail(PSH_EINVAL, "spectrum_level_moments: NULL pointer");
  if (nlevels < 1 || nlevels > psh::kMaxLevels) return fail(PSH_EUNSUPPORTED, "spectrum_level_moments: 1..%d levels", psh::kMaxLevels);
  if (nspec < 1 || nspec > 65535 || m <= 0 || n <= 1) return fail(PSH_EINVAL, "spectrum_level_moments: invalid shape");
  const int nc = n / 2 + 1;
  const int grid = std::min(m, 1024);  // rows are dealt to the blocks; a function of the shape alone
  psh::Scratch partial;
  if (int rc = partial.alloc(static_cast<size_t>(nspec) * grid * psh::kMaxLevels * sizeof(double))) return rc;
  hipLaunchKernelGGL(psh::spectrum_partial, dim3(grid, nspec), dim3(psh::kThreads), 0, c.stream,
                     static_cast<const double2 *>(spec_dev), weights_dev, nlevels, m, nc, (n & 1) == 0 ? 1 : 0,
                     partial.as<double>());
  hipLaunchKernelGGL(psh::spectrum_final, dim3(nlevels, nspec), dim3(psh::kThreads), 0, c.stream,
                     partial.as<const double>(), grid, static_cast<const double2 *>(spec_dev), weights_dev,
                     static_cast<size_t>(m) * nc, static_cast<double>(m) * n, reinterpret_cast<double2 *>(stats_dev));
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}
