// RainFARM stochastic downscaling on the device (pysteps/downscaling/rainfarm.py ``downscale`` without spectral
// fusion), K realisations at once.  float64 throughout like the reference; the uniforms come from rng.hip, the
// transform is psh_fft_irfft2_dev.  (m, n): the low-resolution shape, ds: the factor, (M, N) = (m ds, n ds).
//
//  * psh_rainfarm_spectrum_dev - rainfarm.py:84-97 up to the transform: the Hermitian part of
//    Z = exp(2 pi i u) sqrt(f^-alpha) in rfft2 layout (Re(ifft2(Z)) = irfft2 of it), the DC bin 0
//  * psh_rainfarm_std_dev      - noise.std(): mean, then the mean squared deviation, double-double sums in a fixed order
//  * psh_rainfarm_exp_dev      - rainfarm.py:297-301: E = exp(noise / std) and its ds x ds block means
//  * psh_rainfarm_finish_dev   - rainfarm.py:304-323: E S(precip) / S(block means), the threshold; S is the expansion
//    to the fine grid or its balanced spatial average, summed over coarse cells from a table of kernel-weight
//    partial sums (neither expanded plane exists in memory)
// Every reduction writes block partial sums that one block finishes in a fixed order: the same bits in every run and
// at every position of a plane in a stack.
#include <algorithm>

#include "common.h"
#include "dd.h"

namespace psh {
namespace {

constexpr int kThreads = 256;
constexpr int kPartBlocks = 512;  // partial sums per plane - fixed: the summation order is part of the result

// fftfreq's signed index of bin k of a side of length len
__device__ __forceinline__ int signed_bin(int k, int len) { return k < (len - 1) / 2 + 1 ? k : k - len; }

// one thread per bin (k, l) of the half plane, l <= N / 2; blockIdx.z = realisation.  u: (K, M, N) uniforms.
// vi = 1 / (M (1 / ds)), vj alike: fftfreq's own factor, formed on the host with NumPy's arithmetic.
__global__ __launch_bounds__(kThreads) void spectrum(const double *__restrict__ u, const double *__restrict__ alphas, int M, int N,
                                                     double vi, double vj, double2 *__restrict__ half) {
#pragma clang fp contract(off)
  const int nc = N / 2 + 1;
  const int l = blockIdx.x * kThreads + threadIdx.x;
  const int k = blockIdx.y;
  if (l >= nc) return;
  const size_t p = blockIdx.z;
  const double *up = u + p * static_cast<size_t>(M) * N;
  double2 *hp = half + p * static_cast<size_t>(M) * nc;
  double2 h = make_double2(0.0, 0.0);
  if (k != 0 || l != 0) {
    const double fi = static_cast<double>(signed_bin(k, M)) * vi;
    const double fj = static_cast<double>(signed_bin(l, N)) * vj;
    const double f = sqrt(fi * fi + fj * fj);
    const double amp = sqrt(pow(f, -alphas[p]));  // the same at (-k, -l)
    const int k2 = k ? M - k : 0, l2 = l ? N - l : 0;
    const double two_pi = 2.0 * 3.141592653589793;
    double s1, c1, s2, c2;
    sincos(two_pi * up[static_cast<size_t>(k) * N + l], &s1, &c1);
    sincos(two_pi * up[static_cast<size_t>(k2) * N + l2], &s2, &c2);
    // (Z[k, l] + conj(Z[-k, -l])) / 2; a self-conjugate bin comes out real
    h.x = (c1 * amp + c2 * amp) * 0.5;
    h.y = (s1 * amp - s2 * amp) * 0.5;
  }
  hp[static_cast<size_t>(k) * nc + l] = h;
}

__device__ __forceinline__ dd block_sum(dd v, dd *s_part) {  // valid in thread 0
  v = dd_wave_sum(v);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
  __syncthreads();
  dd t = s_part[0];
  if (threadIdx.x == 0)
    for (int w = 1; w < kThreads / 64; ++w) t = dd_add(t, s_part[w]);
  __syncthreads();
  return t;
}

// partial[p][block] = sum of x (kSquares: of (x - mean[p])^2, the difference rounded as NumPy rounds it, its square exact)
template <bool kSquares>
__global__ __launch_bounds__(kThreads) void std_partial(const double *__restrict__ x, size_t plane, const double2 *__restrict__ stats,
                                                        dd *__restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ dd s_part[kThreads / 64];
  const double *src = x + static_cast<size_t>(blockIdx.y) * plane;
  const double mean = kSquares ? stats[blockIdx.y].x : 0.0;
  dd acc = {0.0, 0.0};
  const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < plane; i += stride) {
    if (kSquares) {
      const double d = src[i] - mean;
      acc = dd_add_sq(acc, d);
    } else {
      acc = dd_add_d(acc, src[i]);
    }
  }
  const dd t = block_sum(acc, s_part);
  if (threadIdx.x == 0) partial[static_cast<size_t>(blockIdx.y) * gridDim.x + blockIdx.x] = t;
}

// stats[p].x = sum / count, or stats[p].y = sqrt(sum / count); one block per plane
template <bool kSquares>
__global__ __launch_bounds__(kThreads) void std_final(const dd *__restrict__ partial, int nblocks, double count,
                                                      double2 *__restrict__ stats) {
  __shared__ dd s_part[kThreads / 64];
  const dd *src = partial + static_cast<size_t>(blockIdx.x) * nblocks;
  dd acc = {0.0, 0.0};
  for (int i = threadIdx.x; i < nblocks; i += kThreads) acc = dd_add(acc, src[i]);
  const dd t = block_sum(acc, s_part);
  if (threadIdx.x == 0) {
    const dd q = dd_div_d(t, count);
    const double v = q.hi + q.lo;
    if (kSquares)
      stats[blockIdx.x].y = sqrt(v);
    else
      stats[blockIdx.x].x = v;
  }
}

// One block: one coarse row I (blockIdx.y) and `cells` coarse cells from blockIdx.x * cells on, of realisation
// blockIdx.z.  A thread owns fine columns: E down the ds rows (coalesced across the threads), their mean into LDS -
// aggregate_fields(axis=0) - then one thread per cell takes the mean of its ds column means - axis=1.
__global__ __launch_bounds__(kThreads) void exp_aggregate(const double *__restrict__ noise, const double2 *__restrict__ stats,
                                                          int m, int n, int ds, int cells, double *__restrict__ e_out,
                                                          double *__restrict__ agg) {
#pragma clang fp contract(off)
  extern __shared__ double s_col[];
  const size_t p = blockIdx.z;
  const int I = blockIdx.y;
  const int J0 = blockIdx.x * cells;
  const int ncell = min(cells, n - J0);
  const int ncols = ncell * ds;
  const size_t N = static_cast<size_t>(n) * ds;
  const size_t base = p * (static_cast<size_t>(m) * ds) * N + (static_cast<size_t>(I) * ds) * N + static_cast<size_t>(J0) * ds;
  const double sd = stats[p].y;
  const double width = static_cast<double>(ds);
  for (int t = threadIdx.x; t < ncols; t += kThreads) {
    double s = 0.0;
    for (int i = 0; i < ds; ++i) {
      const size_t at = base + static_cast<size_t>(i) * N + t;
      const double e = exp(noise[at] / sd);
      e_out[at] = e;
      s = i ? s + e : e;
    }
    s_col[t] = s / width;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < ncell; c += kThreads) {
    double s = s_col[c * ds];
    for (int j = 1; j < ds; ++j) s = s + s_col[c * ds + j];
    agg[p * (static_cast<size_t>(m) * n) + static_cast<size_t>(I) * n + J0 + c] = s / width;
  }
}

// One thread per output pixel (x; y = blockIdx.y; realisation blockIdx.z).  table == nullptr: S is the expansion.
// Else table[(py ds + px)][a][b], a, b < na: the kernel weight that falls into the coarse cell (I + a + amin,
// J + b + amin) from a pixel at phase (py, px) of cell (I, J); cells outside the image are left out of the sums and
// of the weight they are divided by (the reference's convolution of the all-ones mask).
// NA: the table's side when it is known at compile time (3 for every factor the reference's radius rule gives), 0: na.
// A cell outside the image takes part with weight 0 at a clamped index - the sums are those of skipping it, bit for
// bit - so the loads of all cells are independent of each other and of any branch.
template <typename Out, int NA>
__global__ __launch_bounds__(kThreads) void finish(const double *__restrict__ e, const double *__restrict__ precip,
                                                   size_t precip_stride, const double *__restrict__ agg, int m, int n, int ds,
                                                   const double *__restrict__ table, int na, int amin, int has_thr, double thr,
                                                   Out *__restrict__ out) {
#pragma clang fp contract(off)
  const int N = n * ds;
  const int x = blockIdx.x * kThreads + threadIdx.x;
  if (x >= N) return;
  const int y = blockIdx.y;
  const size_t p = blockIdx.z;
  const int I = y / ds, py = y - I * ds;
  const int J = x / ds, px = x - J * ds;
  const double *P = precip + p * precip_stride;
  const double *A = agg + p * (static_cast<size_t>(m) * n);
  const size_t at = p * (static_cast<size_t>(m) * ds) * N + static_cast<size_t>(y) * N + x;
  double norm;
  if (!table) {
    norm = P[static_cast<size_t>(I) * n + J] / A[static_cast<size_t>(I) * n + J];
  } else {
    const int side = NA ? NA : na;
    const double *w = table + (static_cast<size_t>(py) * ds + px) * side * side;
    double sp = 0.0, sa = 0.0, sw = 0.0;
    for (int a = 0; a < side; ++a) {
      const int II = I + a + amin;
      const bool row_in = II >= 0 && II < m;
      const size_t row = static_cast<size_t>(min(max(II, 0), m - 1)) * n;
      for (int b = 0; b < side; ++b) {
        const int JJ = J + b + amin;
        const bool in = row_in && JJ >= 0 && JJ < n;
        const size_t cell = row + min(max(JJ, 0), n - 1);
        const double wv = in ? w[a * side + b] : 0.0;
        sp = sp + wv * P[cell];
        sa = sa + wv * A[cell];
        sw = sw + wv;
      }
    }
    norm = (sp / sw) / (sa / sw);
  }
  double v = e[at] * norm;
  if (has_thr && v < thr) v = 0.0;
  out[at] = static_cast<Out>(v);  // float32: rounded once, here
}

template <typename Out>
void launch_finish(dim3 grid, hipStream_t stream, const double *e, const double *precip, size_t stride, const double *agg, int m,
                   int n, int ds, const double *table, int na, int amin, int has_thr, double thr, Out *out) {
  if (table && na == 3)
    hipLaunchKernelGGL((finish<Out, 3>), grid, dim3(kThreads), 0, stream, e, precip, stride, agg, m, n, ds, table, na, amin, has_thr,
                       thr, out);
  else
    hipLaunchKernelGGL((finish<Out, 0>), grid, dim3(kThreads), 0, stream, e, precip, stride, agg, m, n, ds, table, na, amin, has_thr,
                       thr, out);
}

bool shape_ok(int K, int m, int n, int ds) {
  if (K < 1 || K > 65535 || m < 1 || n < 1 || ds < 1) return false;
  const long long M = static_cast<long long>(m) * ds, N = static_cast<long long>(n) * ds;
  return M <= 65535 && N <= (1 << 24);
}

}  // namespace
}  // namespace psh

using psh::fail;

extern "C" int psh_rainfarm_spectrum_dev(const double *u_dev, const double *alphas_dev, int K, int M, int N, double vi,
                                         double vj, void *half_dev) {
  PSH_ENTER(c);
  if (!u_dev || !alphas_dev || !half_dev) return fail(PSH_EINVAL, "rainfarm_spectrum: NULL pointer");
  if (K < 1 || K > 65535 || M < 1 || M > 65535 || N < 1 || N > (1 << 24)) return fail(PSH_EINVAL, "rainfarm_spectrum: invalid shape");
  const int nc = N / 2 + 1;
  hipLaunchKernelGGL(psh::spectrum, dim3((nc + psh::kThreads - 1) / psh::kThreads, M, K), dim3(psh::kThreads), 0, c.stream, u_dev,
                     alphas_dev, M, N, vi, vj, static_cast<double2 *>(half_dev));
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

extern "C" int psh_rainfarm_std_dev(const double *noise_dev, int K, size_t plane, double *stats_dev) {
  PSH_ENTER(c);
  if (!noise_dev || !stats_dev) return fail(PSH_EINVAL, "rainfarm_std: NULL pointer");
  if (K < 1 || K > 65535 || plane == 0) return fail(PSH_EINVAL, "rainfarm_std: 1..65535 planes, not empty");
  psh::Scratch partial;
  if (int rc = partial.alloc(static_cast<size_t>(K) * psh::kPartBlocks * sizeof(psh::dd))) return rc;
  psh::dd *part = partial.as<psh::dd>();
  double2 *stats = reinterpret_cast<double2 *>(stats_dev);
  const double count = static_cast<double>(plane);
  const dim3 grid(psh::kPartBlocks, K), block(psh::kThreads);
  hipLaunchKernelGGL(psh::std_partial<false>, grid, block, 0, c.stream, noise_dev, plane, static_cast<const double2 *>(stats), part);
  hipLaunchKernelGGL(psh::std_final<false>, dim3(K), block, 0, c.stream, static_cast<const psh::dd *>(part), psh::kPartBlocks, count, stats);
  hipLaunchKernelGGL(psh::std_partial<true>, grid, block, 0, c.stream, noise_dev, plane, static_cast<const double2 *>(stats), part);
  hipLaunchKernelGGL(psh::std_final<true>, dim3(K), block, 0, c.stream, static_cast<const psh::dd *>(part), psh::kPartBlocks, count, stats);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

extern "C" int psh_rainfarm_exp_dev(const double *noise_dev, const double *stats_dev, int K, int m, int n, int ds,
                                    double *e_dev, double *agg_dev) {
  PSH_ENTER(c);
  if (!noise_dev || !stats_dev || !e_dev || !agg_dev) return fail(PSH_EINVAL, "rainfarm_exp: NULL pointer");
  if (!psh::shape_ok(K, m, n, ds) || m > 65535) return fail(PSH_EINVAL, "rainfarm_exp: invalid shape");
  if (ds > 8192) return fail(PSH_EUNSUPPORTED, "rainfarm_exp: ds_factor above 8192");
  const int cells = std::max(1, psh::kThreads / ds);
  const size_t lds = static_cast<size_t>(cells) * ds * sizeof(double);  // <= 64 KiB
  hipLaunchKernelGGL(psh::exp_aggregate, dim3((n + cells - 1) / cells, m, K), dim3(psh::kThreads), lds, c.stream, noise_dev,
                     reinterpret_cast<const double2 *>(stats_dev), m, n, ds, cells, e_dev, agg_dev);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

extern "C" int psh_rainfarm_finish_dev(const double *e_dev, const double *precip_dev, int precip_planes, const double *agg_dev,
                                       int K, int m, int n, int ds, const double *table_dev, int na, int amin, int has_threshold,
                                       double threshold, int f32, void *out_dev) {
  PSH_ENTER(c);
  if (!e_dev || !precip_dev || !agg_dev || !out_dev) return fail(PSH_EINVAL, "rainfarm_finish: NULL pointer");
  if (!psh::shape_ok(K, m, n, ds)) return fail(PSH_EINVAL, "rainfarm_finish: invalid shape");
  if (precip_planes != 1 && precip_planes != K) return fail(PSH_EINVAL, "rainfarm_finish: 1 or K low-resolution planes");
  if (table_dev && (na < 1 || na > 64 || amin > 0 || amin + na - 1 < 0)) return fail(PSH_EINVAL, "rainfarm_finish: invalid table");
  const int M = m * ds, N = n * ds;
  const size_t stride = precip_planes == 1 ? 0 : static_cast<size_t>(m) * n;
  const dim3 grid((N + psh::kThreads - 1) / psh::kThreads, M, K);
  psh::with_real(out_dev, !f32, [&](auto *out) {
    psh::launch_finish(grid, c.stream, e_dev, precip_dev, stride, agg_dev, m, n, ds, table_dev, na, amin, has_threshold, threshold, out);
  });
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}
