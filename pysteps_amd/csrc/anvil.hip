// The ANVIL nowcast (pysteps/nowcasts/anvil.py) on gfx950: moving-window statistics, AR parameters, R(VIL) regression
// and the per-lead-time ARI(p,1) update with the cascade state resident in HBM.
//
// Arithmetic = the reference's NumPy / SciPy expressions, operation by operation, FP contraction off:
//   scipy.ndimage.gaussian_filter(f, sigma, mode="constant") = correlate1d along axis 0, then axis 1, each in float64
//   with the symmetric form of NI_Correlate1D:  o = f[c] w[0]; for j = r .. 1: o += (f[c - j] + f[c + j]) w[j],
//   samples outside the line are the constant 0.0 (added literally; kernels longer than the line included).
//   Several fields built from the same input planes are filtered in one pass (the products x*x, y*y, x*y are formed
//   per sample exactly as NumPy forms them before filtering).
//   _moving_window_corrcoef, adjust_lag2_corrcoef2 and _estimate_ar{1,2}_params: one element-wise kernel; the
//   (1 - g1^2) ** 1.5 term goes through the device's pow, which may differ from the host libm in the last ulp.
//   _r_vil_regression: masking, five filtered fields, the 2 x 2 solve.
//   _update: iterate_ar_model per level (x_new = 0.0 + phi0 x[-1] + phi1 x[-2] + ...), np.sum over the levels in
//   sequence, NaN outside the finite mask, a*v + b or the rain-rate mask, clipping at 0 - one launch per lead time.
#include <algorithm>

#include "common.h"

namespace psh {
namespace {

constexpr int kAnvilThreads = 256;
constexpr int kAnvilMaxRadius = 2048;

// which fields a filter pass forms from its input planes (PSH_ANVIL_RECIPE_* of the header)
enum Recipe { kPlain = 0, kCorr = 1, kRvil = 2, kOnes = 3 };

template <int RECIPE, int NIN, int NF>
__device__ __forceinline__ void fields_at(const double *__restrict__ const *in, size_t at, bool inside, double *f) {
#pragma clang fp contract(off)
  if (!inside) {
#pragma unroll
    for (int k = 0; k < NF; ++k) f[k] = 0.0;
    return;
  }
  if constexpr (RECIPE == kOnes) {
    f[0] = 1.0;
  } else if constexpr (RECIPE == kPlain) {
#pragma unroll
    for (int k = 0; k < NF; ++k) f[k] = in[k][at];
  } else if constexpr (RECIPE == kCorr) {
    // x = in[0], y1 = in[1] (, y2 = in[2]) -> x*x, y1*y1, x*y1 (, y2*y2, x*y2)
    const double x = in[0][at], y1 = in[1][at];
    f[0] = x * x;
    f[1] = y1 * y1;
    f[2] = x * y1;
    if constexpr (NIN == 3) {
      const double y2 = in[2][at];
      f[3] = y2 * y2;
      f[4] = x * y2;
    }
  } else {
    // R(VIL): vil, r, mask -> mask, vil, vil*vil, vil*r, r
    const double v = in[0][at], r = in[1][at], mk = in[2][at];
    f[0] = mk;
    f[1] = v;
    f[2] = v * v;
    f[3] = v * r;
    f[4] = r;
  }
}

// correlate1d down the columns (axis 0) of NF fields formed from NIN planes; 64 x 4 pixels per workgroup, the taps
// read through the caches (all lanes of a wave read the same rows)
template <int RECIPE, int NIN, int NF>
__global__ __launch_bounds__(kAnvilThreads) void anvil_gauss_axis0(const double *__restrict__ in0, const double *__restrict__ in1,
                                                                   const double *__restrict__ in2, int m, int n,
                                                                   const double *__restrict__ w, int r, double *__restrict__ tmp) {
#pragma clang fp contract(off)
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= n || y >= m) return;
  const double *__restrict__ in[3] = {in0, in1, in2};
  const size_t plane = static_cast<size_t>(m) * n;
  double acc[NF], fc[NF];
  fields_at<RECIPE, NIN, NF>(in, static_cast<size_t>(y) * n + x, true, fc);
#pragma unroll
  for (int k = 0; k < NF; ++k) acc[k] = fc[k] * w[0];
  for (int j = r; j >= 1; --j) {
    double fl[NF], fr[NF];
    const int lo = y - j, hi = y + j;
    fields_at<RECIPE, NIN, NF>(in, static_cast<size_t>(lo < 0 ? 0 : lo) * n + x, lo >= 0, fl);
    fields_at<RECIPE, NIN, NF>(in, static_cast<size_t>(hi >= m ? 0 : hi) * n + x, hi < m, fr);
    const double wj = w[j];
#pragma unroll
    for (int k = 0; k < NF; ++k) {
      const double s = fl[k] + fr[k];
      const double p = s * wj;
      acc[k] = acc[k] + p;
    }
  }
#pragma unroll
  for (int k = 0; k < NF; ++k) tmp[k * plane + static_cast<size_t>(y) * n + x] = acc[k];
}

// correlate1d along the rows (axis 1) of nf planes, one after the other; a workgroup stages its 256 outputs' span of
// the row (zeros outside the line) in LDS
__global__ __launch_bounds__(kAnvilThreads) void anvil_gauss_axis1(const double *__restrict__ tmp, int nf, int m, int n,
                                                                   const double *__restrict__ w, int r, double *__restrict__ out) {
#pragma clang fp contract(off)
  extern __shared__ double s_row[];  // [kAnvilThreads + 2 r]
  const int y = blockIdx.y, x0 = blockIdx.x * kAnvilThreads, span = kAnvilThreads + 2 * r;
  const int x = x0 + threadIdx.x, c = threadIdx.x + r;
  const size_t plane = static_cast<size_t>(m) * n;
  for (int f = 0; f < nf; ++f) {
    const double *src = tmp + f * plane + static_cast<size_t>(y) * n;
    if (f) __syncthreads();  // the previous field's taps are read
    for (int i = threadIdx.x; i < span; i += kAnvilThreads) {
      const int s = x0 - r + i;
      s_row[i] = (s >= 0 && s < n) ? src[s] : 0.0;
    }
    __syncthreads();
    if (x < n) {
      double acc = s_row[c] * w[0];
      for (int j = r; j >= 1; --j) {
        const double s = s_row[c - j] + s_row[c + j];
        const double p = s * w[j];
        acc = acc + p;
      }
      out[f * plane + static_cast<size_t>(y) * n + x] = acc;
    }
  }
}

// np.maximum: a NaN in either operand is the result
__device__ __forceinline__ double np_maximum(double a, double b) {
  if (a != a) return a;
  if (b != b) return b;
  return a >= b ? a : b;
}

// _moving_window_corrcoef with zero-mean inputs: cov / (stdx stdy) where the window has data, else 0
__device__ __forceinline__ double window_corr(double nw, double ssx, double ssy, double sxy) {
#pragma clang fp contract(off)
  const double stdx = sqrt(ssx / nw), stdy = sqrt(ssy / nw), cov = sxy / nw;
  const double sxsy = stdx * stdy;
  const bool ok = stdx > 1e-8 && stdy > 1e-8 && sxsy > 1e-8 && nw > 1e-3;
  return ok ? cov / sxsy : 0.0;
}

// per pixel of one cascade level: gamma_1 (, gamma_2 adjusted) -> phi_0 .. phi_p (the reference's zero innovation
// coefficient is not stored).  f = (x*x, y1*y1, x*y1 [, y2*y2, x*y2]) filtered; gamma (ar_order planes) optional
__global__ __launch_bounds__(kAnvilThreads) void anvil_phi(const double *__restrict__ nwin, const double *__restrict__ f, int ar_order,
                                                           size_t count, double *__restrict__ phi, double *__restrict__ gamma) {
#pragma clang fp contract(off)
  const size_t stride = static_cast<size_t>(gridDim.x) * kAnvilThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kAnvilThreads + threadIdx.x; i < count; i += stride) {
    const double nw = nwin[i], ssx = f[i];
    const double g1 = window_corr(nw, ssx, f[count + i], f[2 * count + i]);
    if (ar_order == 1) {
      if (gamma) gamma[i] = g1;
      phi[i] = 1.0 + g1;
      phi[count + i] = -g1;
      continue;
    }
    double g2 = window_corr(nw, ssx, f[3 * count + i], f[4 * count + i]);
    if (gamma) {
      gamma[i] = g1;
      gamma[count + i] = g2;  // overwritten below with the adjusted value when gamma is stored
    }
    // adjust_lag2_corrcoef2
    const double t1 = 2.0 * g1;
    const double t2 = t1 * g2;
    g2 = np_maximum(g2, t2 - 1.0);
    const double g1s = g1 * g1;
    const double a = 3.0 * g1s;
    const double b = a - 2.0;
    const double q = pow(1.0 - g1s, 1.5);
    const double c = 2.0 * q;
    const double d = b + c;
    g2 = np_maximum(g2, d / g1s);
    if (gamma) gamma[count + i] = g2;
    // _estimate_ar2_params
    const double den = 1.0 - g1 * g1;
    const double pd0 = (g1 * (1.0 - g2)) / den;
    const double pd1 = (g2 - g1 * g1) / den;
    phi[i] = 1.0 + pd0;
    phi[count + i] = -pd0 + pd1;
    phi[2 * count + i] = -pd1;
  }
}

// _r_vil_regression, part 1: vil, r -> the masked planes the five filters read (vil, r, mask_obs as 0/1)
__global__ __launch_bounds__(kAnvilThreads) void anvil_rvil_prep(const double *__restrict__ vil, const double *__restrict__ rr, size_t count,
                                                                 double *__restrict__ planes) {
  const size_t stride = static_cast<size_t>(gridDim.x) * kAnvilThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kAnvilThreads + threadIdx.x; i < count; i += stride) {
    double v = vil[i], r = rr[i];
    if (!isfinite(v)) v = 0.0;
    if (!isfinite(r)) r = 0.0;
    const bool obs = v > 10.0 && r > 0.1;
    planes[i] = obs ? v : 0.0;
    planes[count + i] = obs ? r : 0.0;
    planes[2 * count + i] = obs ? 1.0 : 0.0;
  }
}

// _r_vil_regression, part 2: s = (n, sx, sx2, sxy, sy) filtered -> a, b
__global__ __launch_bounds__(kAnvilThreads) void anvil_rvil_solve(const double *__restrict__ vil, const double *__restrict__ s, size_t count,
                                                                  double *__restrict__ a_out, double *__restrict__ b_out) {
#pragma clang fp contract(off)
  const size_t stride = static_cast<size_t>(gridDim.x) * kAnvilThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kAnvilThreads + threadIdx.x; i < count; i += stride) {
    double v = vil[i];
    if (!isfinite(v)) v = 0.0;
    const bool mask_vil = v > 10.0;
    const double m4 = s[i], m2 = s[count + i], m1 = s[2 * count + i], rhs1 = s[3 * count + i], rhs2 = s[4 * count + i];
    const double m3 = m2;
    const double p14 = m1 * m4, p23 = m2 * m3;
    const double det = p14 - p23;
    const double c = 1.0 / det;
    const bool ok = fabs(det) > 1e-8 && m4 > 0.01;
    double a = 0.0, b = 0.0;
    if (ok && mask_vil) {
      const double i11 = c * m4, i12 = -c * m2, i21 = -c * m3, i22 = c * m1;
      const double a1 = i11 * rhs1, a2 = i12 * rhs2, b1 = i21 * rhs1, b2 = i22 * rhs2;
      a = a1 + a2;
      b = b1 + b2;
    }
    a_out[i] = a;
    b_out[i] = b;
  }
}

// finite mask of the advected frames, their zero-filled copies, the rain-rate mask (vil[-1] < 0.1 of the unadvected
// last frame, within the finite mask)
__global__ __launch_bounds__(kAnvilThreads) void anvil_masks(const double *__restrict__ frames, int K, size_t count, double *__restrict__ zeroed,
                                                             unsigned char *__restrict__ mask, unsigned char *__restrict__ rr_mask) {
  const size_t stride = static_cast<size_t>(gridDim.x) * kAnvilThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kAnvilThreads + threadIdx.x; i < count; i += stride) {
    bool fin = true;
    for (int k = 0; k < K; ++k) {
      const double v = frames[k * count + i];
      const bool f = isfinite(v);
      fin = fin && f;
      zeroed[k * count + i] = f ? v : 0.0;
    }
    mask[i] = fin ? 1 : 0;
    if (rr_mask) rr_mask[i] = (fin && frames[(K - 1) * count + i] < 0.1) ? 1 : 0;
  }
}

// np.diff of two cascade planes with non-finite differences set to 0
__global__ __launch_bounds__(kAnvilThreads) void anvil_diff(const double *__restrict__ older, const double *__restrict__ newer, size_t count,
                                                            double *__restrict__ out) {
#pragma clang fp contract(off)
  const size_t stride = static_cast<size_t>(gridDim.x) * kAnvilThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kAnvilThreads + threadIdx.x; i < count; i += stride) {
    const double d = newer[i] - older[i];
    out[i] = isfinite(d) ? d : 0.0;
  }
}

// one lead time: ring (L, P, m, n) with the oldest slot at `head`; phi (L, P, m, n)
template <int P>
__global__ __launch_bounds__(kAnvilThreads) void anvil_update(double *__restrict__ ring, const double *__restrict__ phi, int L, size_t count,
                                                              int head, const unsigned char *__restrict__ mask,
                                                              const unsigned char *__restrict__ rr_mask, const double *__restrict__ ra,
                                                              const double *__restrict__ rb, double *__restrict__ out) {
#pragma clang fp contract(off)
  const size_t stride = static_cast<size_t>(gridDim.x) * kAnvilThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kAnvilThreads + threadIdx.x; i < count; i += stride) {
    double sum = 0.0;
    for (int l = 0; l < L; ++l) {
      double *rg = ring + static_cast<size_t>(l) * P * count;
      const double *ph = phi + static_cast<size_t>(l) * P * count;
      double xn = 0.0;
#pragma unroll
      for (int t = 0; t < P; ++t) {
        const int slot = (head + P - 1 - t) % P;  // x[-(t + 1)]
        const double p = ph[t * count + i] * rg[slot * count + i];
        xn = xn + p;
      }
      rg[head * count + i] = xn;
      sum = l == 0 ? xn : sum + xn;
    }
    double v = mask[i] ? sum : static_cast<double>(NAN);
    if (ra) {
      const double av = ra[i] * v;
      v = av + rb[i];
    } else if (rr_mask && rr_mask[i]) {
      v = 0.0;
    }
    if (v < 0.0) v = 0.0;
    out[i] = v;
  }
}

unsigned grid_for(size_t count) {
  return static_cast<unsigned>(std::max<size_t>(1, std::min<size_t>((count + kAnvilThreads - 1) / kAnvilThreads, 16384)));
}

template <int RECIPE, int NIN, int NF>
void launch_axis0(const double *in0, const double *in1, const double *in2, int m, int n, const double *w, int r, double *tmp,
                  hipStream_t s) {
  const dim3 grid((n + 63) / 64, (m + 3) / 4);
  hipLaunchKernelGGL((anvil_gauss_axis0<RECIPE, NIN, NF>), grid, dim3(kAnvilThreads), 0, s, in0, in1, in2, m, n, w, r, tmp);
}

int gauss(const double *in0, const double *in1, const double *in2, int recipe, int m, int n, const double *weights_host, int r,
          double *out, hipStream_t s) {
  int nin = 0, nf = 0;
  switch (recipe) {
    case kPlain: nin = in2 ? 3 : in1 ? 2 : 1; nf = nin; break;
    case kCorr: nin = in2 ? 3 : 2; nf = in2 ? 5 : 3; break;
    case kRvil: nin = 3; nf = 5; break;
    default: nin = 0; nf = 1; break;
  }
  const size_t plane = static_cast<size_t>(m) * n;
  const size_t wbytes = (static_cast<size_t>(r + 1) * sizeof(double) + 255) & ~static_cast<size_t>(255);
  psh::Scratch blk;
  if (int rc = blk.alloc(wbytes + static_cast<size_t>(nf) * plane * sizeof(double))) return rc;
  double *w = blk.as<double>();
  double *tmp = blk.at<double>(wbytes);
  // (the caller's weights may go once this call returns: the copy is waited for)
  PSH_HIP(hipMemcpyAsync(w, weights_host, static_cast<size_t>(r + 1) * sizeof(double), hipMemcpyHostToDevice, s));
  PSH_HIP(hipStreamSynchronize(s));
  switch (recipe * 4 + nin) {
    case kPlain * 4 + 1: launch_axis0<kPlain, 1, 1>(in0, in1, in2, m, n, w, r, tmp, s); break;
    case kPlain * 4 + 2: launch_axis0<kPlain, 2, 2>(in0, in1, in2, m, n, w, r, tmp, s); break;
    case kPlain * 4 + 3: launch_axis0<kPlain, 3, 3>(in0, in1, in2, m, n, w, r, tmp, s); break;
    case kCorr * 4 + 2: launch_axis0<kCorr, 2, 3>(in0, in1, in2, m, n, w, r, tmp, s); break;
    case kCorr * 4 + 3: launch_axis0<kCorr, 3, 5>(in0, in1, in2, m, n, w, r, tmp, s); break;
    case kRvil * 4 + 3: launch_axis0<kRvil, 3, 5>(in0, in1, in2, m, n, w, r, tmp, s); break;
    default: launch_axis0<kOnes, 0, 1>(in0, in1, in2, m, n, w, r, tmp, s); break;
  }
  const size_t lds = static_cast<size_t>(kAnvilThreads + 2 * r) * sizeof(double);
  hipLaunchKernelGGL(anvil_gauss_axis1, dim3((n + kAnvilThreads - 1) / kAnvilThreads, m), dim3(kAnvilThreads), lds, s,
                     static_cast<const double *>(tmp), nf, m, n, static_cast<const double *>(w), r, out);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

int check_shape(const char *what, int m, int n) {
  if (m <= 0 || n <= 0 || m > 65535 || static_cast<size_t>(m) * n > (size_t(1) << 30))
    return fail(PSH_EINVAL, "%s: invalid shape (%d,%d)", what, m, n);
  return PSH_OK;
}

}  // namespace
}  // namespace psh

using psh::fail;

extern "C" int psh_anvil_gauss_dev(const double *in0_dev, const double *in1_dev, const double *in2_dev, int recipe, int m, int n,
                                   const double *weights_host, int radius, double *out_dev) {
  using namespace psh;
  PSH_ENTER(c);
  if (int rc = check_shape("anvil_gauss", m, n)) return rc;
  if (!weights_host || !out_dev) return fail(PSH_EINVAL, "anvil_gauss: NULL pointer");
  if (radius < 0 || radius > kAnvilMaxRadius) return fail(PSH_EUNSUPPORTED, "anvil_gauss: kernel radius %d (0..%d)", radius, kAnvilMaxRadius);
  const bool ok = (recipe == kPlain && in0_dev && (in1_dev || !in2_dev)) || (recipe == kCorr && in0_dev && in1_dev) ||
                  (recipe == kRvil && in0_dev && in1_dev && in2_dev) || (recipe == kOnes && !in0_dev && !in1_dev && !in2_dev);
  if (!ok) return fail(PSH_EINVAL, "anvil_gauss: recipe %d does not take these inputs", recipe);
  return gauss(in0_dev, in1_dev, in2_dev, recipe, m, n, weights_host, radius, out_dev, c.stream);
}

extern "C" int psh_anvil_phi_dev(const double *nwin_dev, const double *fields_dev, int ar_order, int m, int n, double *phi_dev,
                                 double *gamma_dev) {
  using namespace psh;
  PSH_ENTER(c);
  if (int rc = check_shape("anvil_phi", m, n)) return rc;
  if (!nwin_dev || !fields_dev || !phi_dev) return fail(PSH_EINVAL, "anvil_phi: NULL pointer");
  if (ar_order != 1 && ar_order != 2) return fail(PSH_EUNSUPPORTED, "anvil_phi: ar_order %d (1 or 2)", ar_order);
  const size_t count = static_cast<size_t>(m) * n;
  hipLaunchKernelGGL(anvil_phi, dim3(grid_for(count)), dim3(kAnvilThreads), 0, c.stream, nwin_dev, fields_dev, ar_order, count, phi_dev,
                     gamma_dev);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

extern "C" int psh_anvil_rvil_dev(const double *vil_dev, const double *rainrate_dev, int m, int n, const double *weights_host,
                                  int radius, double *a_dev, double *b_dev) {
  using namespace psh;
  PSH_ENTER(c);
  if (int rc = check_shape("anvil_rvil", m, n)) return rc;
  if (!vil_dev || !rainrate_dev || !weights_host || !a_dev || !b_dev) return fail(PSH_EINVAL, "anvil_rvil: NULL pointer");
  if (radius < 0 || radius > kAnvilMaxRadius) return fail(PSH_EUNSUPPORTED, "anvil_rvil: kernel radius %d (0..%d)", radius, kAnvilMaxRadius);
  const size_t count = static_cast<size_t>(m) * n;
  psh::Scratch blk;
  if (int rc = blk.alloc(8 * count * sizeof(double))) return rc;
  double *planes = blk.as<double>(), *sums = planes + 3 * count;
  hipLaunchKernelGGL(anvil_rvil_prep, dim3(grid_for(count)), dim3(kAnvilThreads), 0, c.stream, vil_dev, rainrate_dev, count, planes);
  PSH_HIP(hipGetLastError());
  if (int rc = gauss(planes, planes + count, planes + 2 * count, kRvil, m, n, weights_host, radius, sums, c.stream)) return rc;
  hipLaunchKernelGGL(anvil_rvil_solve, dim3(grid_for(count)), dim3(kAnvilThreads), 0, c.stream, vil_dev,
                     static_cast<const double *>(sums), count, a_dev, b_dev);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

extern "C" int psh_anvil_masks_dev(const double *frames_dev, int K, int m, int n, double *zeroed_dev, unsigned char *mask_dev,
                                   unsigned char *rr_mask_dev) {
  using namespace psh;
  PSH_ENTER(c);
  if (int rc = check_shape("anvil_masks", m, n)) return rc;
  if (!frames_dev || !zeroed_dev || !mask_dev) return fail(PSH_EINVAL, "anvil_masks: NULL pointer");
  if (K < 1 || K > 64) return fail(PSH_EINVAL, "anvil_masks: %d frames", K);
  const size_t count = static_cast<size_t>(m) * n;
  hipLaunchKernelGGL(anvil_masks, dim3(grid_for(count)), dim3(kAnvilThreads), 0, c.stream, frames_dev, K, count, zeroed_dev, mask_dev,
                     rr_mask_dev);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

extern "C" int psh_anvil_diff_dev(const double *older_dev, const double *newer_dev, size_t count, double *out_dev) {
  using namespace psh;
  PSH_ENTER(c);
  if (!older_dev || !newer_dev || !out_dev) return fail(PSH_EINVAL, "anvil_diff: NULL pointer");
  if (count == 0) return PSH_OK;
  hipLaunchKernelGGL(anvil_diff, dim3(grid_for(count)), dim3(kAnvilThreads), 0, c.stream, older_dev, newer_dev, count, out_dev);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

extern "C" int psh_anvil_update_dev(double *ring_dev, const double *phi_dev, int n_levels, int p, int head, int m, int n,
                                    const unsigned char *mask_dev, const unsigned char *rr_mask_dev, const double *a_dev,
                                    const double *b_dev, double *out_dev) {
  using namespace psh;
  PSH_ENTER(c);
  if (int rc = check_shape("anvil_update", m, n)) return rc;
  if (!ring_dev || !phi_dev || !mask_dev || !out_dev || (a_dev == nullptr) != (b_dev == nullptr))
    return fail(PSH_EINVAL, "anvil_update: NULL pointer");
  if (n_levels < 1 || n_levels > 64) return fail(PSH_EINVAL, "anvil_update: %d levels", n_levels);
  if (p != 2 && p != 3) return fail(PSH_EUNSUPPORTED, "anvil_update: %d AR terms (2 or 3)", p);
  if (head < 0 || head >= p) return fail(PSH_EINVAL, "anvil_update: ring head %d of %d slots", head, p);
  const size_t count = static_cast<size_t>(m) * n;
  if (p == 2)
    hipLaunchKernelGGL(anvil_update<2>, dim3(grid_for(count)), dim3(kAnvilThreads), 0, c.stream, ring_dev, phi_dev, n_levels, count, head,
                       mask_dev, rr_mask_dev, a_dev, b_dev, out_dev);
  else
    hipLaunchKernelGGL(anvil_update<3>, dim3(grid_for(count)), dim3(kAnvilThreads), 0, c.stream, ring_dev, phi_dev, n_levels, count, head,
                       mask_dev, rr_mask_dev, a_dev, b_dev, out_dev);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}
