// Short-space Fourier (ssft / nested) noise on the device: the windowed filter bank and the composite of
// pysteps/noise/fftgenerators.py:442-852 (initialize_nonparam_2d_ssft_filter, initialize_nonparam_2d_nested_filter,
// generate_noise_2d_ssft_filter).  float64 throughout like the reference; every call is queued on the library stream.
//
// The reference's filters are real full-spectrum planes F and its generator forms Re(ifft2(fft2(N) F)) with N real:
// that is irfft2 of the rfft2-layout half of fft2(N) Fs, Fs(k) = (F(k) + F(-k)) / 2, so filters are kept as
// (m, n/2+1) half planes - one rfft2 of the white noise and one irfft2 per DISTINCT plane (windows that did not pass
// the wet-area test share the global one).  Windows are rectangles [i0, i1) x [j0, j1) with a mask tile of their own
// shape; the passes here read and write the rectangles only.
//
//  * psh_ssft_war_counts_dev     - the count of field * mask > 0.01 per window, all windows in one launch (integers)
//  * psh_ssft_local_filters_dev  - per window: field[f] * mask prepared as the reference's inner initialiser prepares
//    it, rfft2 averaged over f, real and imaginary parts standardised by their full-plane mean and population std (read
//    off the half plane), abs, the self-mirrored columns made symmetric
//  * psh_ssft_merge_dev          - the nested initialiser's F = F w + new (1 - w)
//  * psh_ssft_generate_dev       - K white-noise planes -> K composites: spectrum x plane inside the inverse transform,
//    cN += flN M rectangle by rectangle, cN / sM where sM > 0, (cN - mean) / std
//
// A window table holds 6 int64 per window: {i0, i1, j0, j1, tile, plane} - tile: the element offset of the window's
// (i1 - i0, j1 - j0) mask tile in the tile array, negative for a mask of ones; plane: the filter plane the window
// writes (local filters) or uses (generator).  Every reduction writes block partial sums that one block finishes in a
// fixed order, and a pixel's windows are added in a fixed order (planes as the table first names them, a plane's
// windows by table position - the numbering of the planes does not enter): the same bits in
// every run, for every K and at every position of a plane in a batch.
#include <algorithm>
#include <vector>

#include "common.h"
#include "dd.h"

namespace psh {
namespace {

constexpr int kThreads = 256;
constexpr int kRowBlocks = 256;  // partial sums per half plane - fixed: the summation order is part of the result
constexpr int kWinFields = 6;
constexpr int kMinBlocks = 64;  // blocks per field of the preparation's minima

struct Win {
  int i0, i1, j0, j1;
  long long tile;  // < 0: ones
  int plane;
};

// blockIdx.y = window; the window's pixels of every field are dealt to the block's threads
__global__ __launch_bounds__(kThreads) void war_counts(const double *__restrict__ fields, int nr_fields, size_t plane, int n,
                                                       const long long *__restrict__ wins, const double *__restrict__ tiles,
                                                       unsigned long long *__restrict__ counts) {
  const long long *w = wins + static_cast<size_t>(blockIdx.y) * kWinFields;
  const int i0 = static_cast<int>(w[0]), i1 = static_cast<int>(w[1]), j0 = static_cast<int>(w[2]), j1 = static_cast<int>(w[3]);
  const double *tile = w[4] >= 0 ? tiles + w[4] : nullptr;
  const int width = j1 - j0;
  const size_t area = static_cast<size_t>(i1 - i0) * width;
  const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
  unsigned c = 0;
  for (int f = 0; f < nr_fields; ++f) {
    const double *src = fields + static_cast<size_t>(f) * plane;
    for (size_t t = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; t < area; t += stride) {
      const int r = static_cast<int>(t / width), col = static_cast<int>(t - static_cast<size_t>(r) * width);
      const double v = src[static_cast<size_t>(i0 + r) * n + j0 + col] * (tile ? tile[t] : 1.0);  // one rounded product
      c += v > 0.01 ? 1u : 0u;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(counts + blockIdx.y, static_cast<unsigned long long>(c));  // integers: exact in any order
}

// The field a local filter is taken of.  The reference hands g = field * mask (the global filter: g = field, the
// tapering applied afterwards) to initialize_nonparam_2d_fft_filter, which prepares it once more with its own defaults
// (fftgenerators.py:282-299): over the whole stack g[g > g.min()] -= g[g > g.min()].min() - g.min(), then every
// field's own minimum is subtracted.  stats = {g.min(), min of g above it, the fields' minima after the shift}; the
// minima are exact in any order.  Outside the rectangle g = field * 0.
__device__ __forceinline__ double tile_at(const Win &w, const double *tiles, int r, int c) {
  return w.tile >= 0 ? tiles[w.tile + static_cast<size_t>(r) * (w.j1 - w.j0) + c] : 1.0;
}

__device__ __forceinline__ double shifted(double g, double gmin, double shift) { return g > gmin ? g - shift : g; }

__device__ __forceinline__ double block_min(double v, double *s_part) {  // valid in thread 0
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = fmin(v, __shfl_xor(v, d));
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = s_part[0];
  if (threadIdx.x == 0)
    for (int k = 1; k < kThreads / 64; ++k) t = fmin(t, s_part[k]);
  __syncthreads();
  return t;
}

// kMode 0: min g; 1: min of g above stats[0]; 2: min of the shifted g.  blockIdx.y = field; the rectangle's pixels are
// dealt to the blocks, the pixels outside it (g = +0, the field being finite) enter as one value.
template <int kMode>
__global__ __launch_bounds__(kThreads) void window_min(const double *__restrict__ fields, size_t plane, int n, Win w,
                                                       const double *__restrict__ tiles, int taper_after,
                                                       const double *__restrict__ stats, double *__restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ double s_part[kThreads / 64];
  const double *src = fields + static_cast<size_t>(blockIdx.y) * plane;
  const double gmin = kMode >= 1 ? stats[0] : 0.0;
  const double shift = kMode == 2 ? stats[1] - stats[0] : 0.0;
  const int width = w.j1 - w.j0;
  const size_t area = static_cast<size_t>(w.i1 - w.i0) * width;
  const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
  double best = INFINITY;
  auto take = [&](double g) {
    if (kMode == 0) best = fmin(best, g);
    if (kMode == 1 && g > gmin) best = fmin(best, g);
    if (kMode == 2) best = fmin(best, shifted(g, gmin, shift));
  };
  if (area < plane && blockIdx.x == 0 && threadIdx.x == 0) take(0.0);
  for (size_t t = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; t < area; t += stride) {
    const int r = static_cast<int>(t / width), c = static_cast<int>(t - static_cast<size_t>(r) * width);
    const double v = src[static_cast<size_t>(w.i0 + r) * n + w.j0 + c];
    take(taper_after ? v : v * tile_at(w, tiles, r, c));
  }
  const double t = block_min(best, s_part);
  if (threadIdx.x == 0) partial[static_cast<size_t>(blockIdx.y) * gridDim.x + blockIdx.x] = t;
}

// out[blockIdx.x] = min of `per` consecutive partials
__global__ __launch_bounds__(kThreads) void window_min_final(const double *__restrict__ partial, int per, double *__restrict__ out) {
  __shared__ double s_part[kThreads / 64];
  double best = INFINITY;
  for (int i = threadIdx.x; i < per; i += kThreads) best = fmin(best, partial[static_cast<size_t>(blockIdx.x) * per + i]);
  const double t = block_min(best, s_part);
  if (threadIdx.x == 0) out[blockIdx.x] = t;
}

// out = the prepared g of field blockIdx.z over the whole plane (times the tile when it tapers afterwards); blockIdx.y = row
__global__ __launch_bounds__(kThreads) void masked_field(const double *__restrict__ fields, size_t plane, int n, Win w,
                                                         const double *__restrict__ tiles, int taper_after,
                                                         const double *__restrict__ stats, int field, double *__restrict__ out) {
#pragma clang fp contract(off)
  const int x = blockIdx.x * kThreads + threadIdx.x;
  if (x >= n) return;
  const int y = blockIdx.y;
  const bool inside = y >= w.i0 && y < w.i1 && x >= w.j0 && x < w.j1;
  const double mask = inside ? tile_at(w, tiles, y - w.i0, x - w.j0) : 0.0;
  const size_t at = static_cast<size_t>(y) * n + x;
  const double v = fields[static_cast<size_t>(field) * plane + at];
  const double g = taper_after ? v : v * mask;
  const double h = shifted(g, stats[0], stats[1] - stats[0]) - stats[2 + field];
  out[at] = taper_after ? h * mask : h;
}

// acc += add, then acc *= scale where scale != 1 (F += fft2(...); F /= nr_fields: NumPy divides a complex array by
// the real count through the reciprocal)
__global__ __launch_bounds__(kThreads) void spectrum_add(double2 *__restrict__ acc, const double2 *__restrict__ add, size_t count,
                                                         double scale) {
#pragma clang fp contract(off)
  const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < count; i += stride) {
    double2 a = acc[i];
    const double2 b = add[i];
    a.x = a.x + b.x;
    a.y = a.y + b.y;
    if (scale != 1.0) {
      a.x = a.x * scale;
      a.y = a.y * scale;
    }
    acc[i] = a;
  }
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

// Moments of the real and of the imaginary parts over the FULL (m, n) plane, from its rfft2 half: a column with a
// mirror column stands for two bins, the mirror's imaginary part with the sign flipped.  partial[block] = {re, im}:
// the sums (kSquares: of the squared deviations from stats' means).  Rows are dealt to the blocks.
template <bool kSquares>
__global__ __launch_bounds__(kThreads) void half_partial(const double2 *__restrict__ spec, int m, int nc, int n_even,
                                                         const double *__restrict__ stats, dd *__restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ dd s_part[kThreads / 64];
  const double mean_re = kSquares ? stats[0] : 0.0, mean_im = kSquares ? stats[2] : 0.0;
  dd re = {0.0, 0.0}, im = {0.0, 0.0};
  for (int r = blockIdx.x; r < m; r += gridDim.x) {
    for (int c = threadIdx.x; c < nc; c += kThreads) {
      const double2 v = spec[static_cast<size_t>(r) * nc + c];
      const bool mirrored = !(c == 0 || (n_even && c == nc - 1));
      if (kSquares) {
        const double dr = v.x - mean_re, di = v.y - mean_im;
        re = dd_add_sq(re, dr);
        im = dd_add_sq(im, di);
        if (mirrored) {
          const double dm = -v.y - mean_im;
          re = dd_add_sq(re, dr);
          im = dd_add_sq(im, dm);
        }
      } else {
        re = dd_add_d(re, mirrored ? v.x * 2.0 : v.x);
        if (!mirrored) im = dd_add_d(im, v.y);  // a mirrored pair adds y and -y
      }
    }
  }
  const dd tr = block_sum(re, s_part);
  const dd ti = block_sum(im, s_part);
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x] = tr;
    partial[2 * blockIdx.x + 1] = ti;
  }
}

// stats = {mean_re, std_re, mean_im, std_im}; one block
template <bool kSquares>
__global__ __launch_bounds__(kThreads) void half_final(const dd *__restrict__ partial, int nblocks, double count,
                                                       double *__restrict__ stats) {
  __shared__ dd s_part[kThreads / 64];
  dd re = {0.0, 0.0}, im = {0.0, 0.0};
  for (int i = threadIdx.x; i < nblocks; i += kThreads) {
    re = dd_add(re, partial[2 * i]);
    im = dd_add(im, partial[2 * i + 1]);
  }
  const dd tr = block_sum(re, s_part);
  const dd ti = block_sum(im, s_part);
  if (threadIdx.x == 0) {
    const dd qr = dd_div_d(tr, count), qi = dd_div_d(ti, count);
    const double vr = qr.hi + qr.lo, vi = qi.hi + qi.lo;
    if (kSquares) {
      stats[1] = sqrt(vr);
      stats[3] = sqrt(vi);
    } else {
      stats[0] = vr;
      stats[2] = vi;
    }
  }
}

// fftgenerators.py:316-324: each part standardised where its std > 0, then np.abs
__global__ __launch_bounds__(kThreads) void standardise_abs(const double2 *__restrict__ spec, size_t count,
                                                            const double *__restrict__ stats, double *__restrict__ out) {
#pragma clang fp contract(off)
  const double mean_re = stats[0], std_re = stats[1], mean_im = stats[2], std_im = stats[3];
  const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < count; i += stride) {
    double2 v = spec[i];
    if (std_im > 0.0) v.y = (v.y - mean_im) / std_im;
    if (std_re > 0.0) v.x = (v.x - mean_re) / std_re;
    out[i] = hypot(v.x, v.y);
  }
}

// The two columns of a half plane that are their own mirror images (kx = 0 and, for even n, the Nyquist column) hold
// F(ky) and F(-ky) both: each pair takes its mean, (F(k) + F(-k)) / 2 as on every other bin of the folded plane, so
// that the plane expanded to the full spectrum and folded again is the same plane bit for bit.
__global__ __launch_bounds__(kThreads) void symmetrise_columns(double *__restrict__ plane, int m, int nc, int n_even) {
#pragma clang fp contract(off)
  const int r = 1 + blockIdx.x * kThreads + threadIdx.x;
  const int c = blockIdx.y == 0 ? 0 : nc - 1;
  if (blockIdx.y == 1 && !n_even) return;
  if (r >= m - r) return;  // r == m - r: its own mirror
  const size_t a = static_cast<size_t>(r) * nc + c, b = static_cast<size_t>(m - r) * nc + c;
  const double mean = (plane[a] + plane[b]) / 2.0;
  plane[a] = mean;
  plane[b] = mean;
}

// fftgenerators.py:708-725 on a half plane: newfilter *= 1 - w; F *= w; F += newfilter
__global__ __launch_bounds__(kThreads) void merge(double *__restrict__ F, const double *__restrict__ w,
                                                  const double *__restrict__ fresh, size_t count) {
#pragma clang fp contract(off)
  const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < count; i += stride) {
    const double wi = w[i];
    const double keep = F[i] * wi;
    const double add = fresh[i] * (1.0 - wi);
    F[i] = keep + add;
  }
}

// cN += flN * M inside one window's rectangle; blockIdx.y = row of the rectangle, blockIdx.z = member
__global__ __launch_bounds__(kThreads) void accumulate(const double *__restrict__ flN, size_t plane, int n, Win w,
                                                       const double *__restrict__ tiles, double *__restrict__ cN) {
#pragma clang fp contract(off)
  const int width = w.j1 - w.j0;
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c >= width) return;
  const int r = blockIdx.y;
  const size_t at = static_cast<size_t>(blockIdx.z) * plane + static_cast<size_t>(w.i0 + r) * n + w.j0 + c;
  const double mask = w.tile >= 0 ? tiles[w.tile + static_cast<size_t>(r) * width + c] : 1.0;
  const double term = flN[at] * mask;
  cN[at] = cN[at] + term;
}

// cN[sM > 0] /= sM[sM > 0]; blockIdx.y = member
__global__ __launch_bounds__(kThreads) void divide_by_masks(double *__restrict__ cN, size_t plane, const double *__restrict__ sM) {
  double *x = cN + static_cast<size_t>(blockIdx.y) * plane;
  const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < plane; i += stride) {
    const double s = sM[i];
    if (s > 0.0) x[i] = x[i] / s;
  }
}

// (cN - cN.mean()) / cN.std(); blockIdx.y = member
__global__ __launch_bounds__(kThreads) void standardise(double *__restrict__ cN, size_t plane, const double2 *__restrict__ stats) {
#pragma clang fp contract(off)
  double *x = cN + static_cast<size_t>(blockIdx.y) * plane;
  const double mean = stats[blockIdx.y].x, sd = stats[blockIdx.y].y;
  const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < plane; i += stride) x[i] = (x[i] - mean) / sd;
}

unsigned sweep_blocks(size_t n) {
  const size_t blocks = (n + kThreads - 1) / kThreads;
  return static_cast<unsigned>(blocks < 2048 ? (blocks ? blocks : 1) : 2048);
}

// the table's rows as Win, every rectangle inside the image, every tile inside the tile array, every plane < nplanes
int read_windows(const char *what, const long long *wins_host, int nwin, int m, int n, size_t tiles_count, bool has_tiles,
                 int nplanes, std::vector<Win> *out) {
  out->resize(nwin);
  for (int k = 0; k < nwin; ++k) {
    const long long *w = wins_host + static_cast<size_t>(k) * kWinFields;
    if (w[0] < 0 || w[1] < w[0] || w[1] > m || w[2] < 0 || w[3] < w[2] || w[3] > n)
      return fail(PSH_EINVAL, "%s: window %d [%lld, %lld) x [%lld, %lld) does not lie in (%d, %d)", what, k, w[0], w[1], w[2], w[3], m, n);
    const unsigned long long area = static_cast<unsigned long long>(w[1] - w[0]) * static_cast<unsigned long long>(w[3] - w[2]);
    if (w[4] >= 0 && (!has_tiles || static_cast<unsigned long long>(w[4]) + area > tiles_count))
      return fail(PSH_EINVAL, "%s: the mask tile of window %d does not lie in the tile array", what, k);
    if (w[5] < 0 || w[5] >= nplanes) return fail(PSH_EINVAL, "%s: window %d names plane %lld of %d", what, k, w[5], nplanes);
    (*out)[k] = {static_cast<int>(w[0]), static_cast<int>(w[1]), static_cast<int>(w[2]), static_cast<int>(w[3]), w[4],
                 static_cast<int>(w[5])};
  }
  return PSH_OK;
}

bool shape_ok(int m, int n) { return fft_shape_supported(m, n); }

}  // namespace
}  // namespace psh

using psh::fail;

extern "C" int psh_ssft_war_counts_dev(const double *fields_dev, int nr_fields, int m, int n, const long long *wins_host,
                                       int nwin, const double *tiles_dev, size_t tiles_count,
                                       unsigned long long *counts_dev) {
  PSH_ENTER(c);
  if (!fields_dev || !wins_host || !counts_dev) return fail(PSH_EINVAL, "ssft_war_counts: NULL pointer");
  if (nr_fields < 1 || m < 1 || n < 1 || m > 65535 || n > 65535) return fail(PSH_EINVAL, "ssft_war_counts: invalid shape");
  if (nwin < 1 || nwin > 65535) return fail(PSH_EINVAL, "ssft_war_counts: 1..65535 windows");
  std::vector<psh::Win> wins;
  if (int rc = psh::read_windows("ssft_war_counts", wins_host, nwin, m, n, tiles_count, tiles_dev != nullptr, 1 << 30, &wins)) return rc;
  psh::Scratch table;
  const size_t bytes = static_cast<size_t>(nwin) * psh::kWinFields * sizeof(long long);
  if (int rc = table.alloc(bytes)) return rc;
  PSH_HIP(hipMemcpyAsync(table.as<void>(), wins_host, bytes, hipMemcpyHostToDevice, c.stream));  // pageable: staged before the return
  PSH_HIP(hipMemsetAsync(counts_dev, 0, static_cast<size_t>(nwin) * sizeof(unsigned long long), c.stream));
  size_t largest = 1;
  for (const psh::Win &w : wins) largest = std::max(largest, static_cast<size_t>(w.i1 - w.i0) * (w.j1 - w.j0));
  const unsigned bx = std::min(psh::sweep_blocks(largest), 64u);
  hipLaunchKernelGGL(psh::war_counts, dim3(bx, nwin), dim3(psh::kThreads), 0, c.stream, fields_dev, nr_fields,
                     static_cast<size_t>(m) * n, n, table.as<const long long>(), tiles_dev, counts_dev);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

extern "C" int psh_ssft_local_filters_dev(const double *fields_dev, int nr_fields, int m, int n, const long long *wins_host,
                                          int nwin, const double *tiles_dev, size_t tiles_count, int taper_after, int nplanes,
                                          double *planes_dev) {
  PSH_ENTER(c);
  if (!fields_dev || !wins_host || !planes_dev) return fail(PSH_EINVAL, "ssft_local_filters: NULL pointer");
  if (nr_fields < 1 || nr_fields > 65535 || nwin < 1 || nplanes < 1)
    return fail(PSH_EINVAL, "ssft_local_filters: 1..65535 fields, at least one window and plane");
  if (!psh::shape_ok(m, n))
    return fail(PSH_EUNSUPPORTED, "ssft_local_filters: (%d,%d) - sides: powers of two up to 8192 or any length up to 4096", m, n);
  std::vector<psh::Win> wins;
  if (int rc = psh::read_windows("ssft_local_filters", wins_host, nwin, m, n, tiles_count, tiles_dev != nullptr, nplanes, &wins)) return rc;
  const int nc = n / 2 + 1;
  const size_t plane = static_cast<size_t>(m) * n, half = static_cast<size_t>(m) * nc;
  const size_t spec_bytes = half * sizeof(double2), part_bytes = 2 * psh::kRowBlocks * sizeof(psh::dd);
  const size_t min_bytes = static_cast<size_t>(nr_fields) * psh::kMinBlocks * sizeof(double);
  const size_t prep_bytes = (2 + static_cast<size_t>(nr_fields)) * sizeof(double);
  psh::Scratch blk;
  if (int rc = blk.alloc(plane * sizeof(double) + 2 * spec_bytes + part_bytes + 4 * sizeof(double) + min_bytes + prep_bytes)) return rc;
  double2 *acc = blk.as<double2>();  // the 16-byte types first: they stay aligned whatever the plane's size
  double2 *one = blk.at<double2>(spec_bytes);
  psh::dd *partial = blk.at<psh::dd>(2 * spec_bytes);
  double *masked = blk.at<double>(2 * spec_bytes + part_bytes);
  double *stats = masked + plane;
  double *min_part = stats + 4;
  double *prep = min_part + static_cast<size_t>(nr_fields) * psh::kMinBlocks;
  const dim3 block(psh::kThreads), image((n + psh::kThreads - 1) / psh::kThreads, m), mins(psh::kMinBlocks, nr_fields);
  const int rows = std::min(m, psh::kRowBlocks);
  const double cells = static_cast<double>(m) * static_cast<double>(n);
  const int n_even = (n & 1) == 0 ? 1 : 0;
  const int after = taper_after ? 1 : 0;
  for (const psh::Win &w : wins) {
    if (after && (w.i0 != 0 || w.j0 != 0 || w.i1 != m || w.j1 != n))
      return fail(PSH_EINVAL, "ssft_local_filters: tapering after the preparation is for the whole-domain window");
    // the second preparation: g.min(), the smallest g above it, every field's minimum after the shift
    const double *cprep = prep;
    hipLaunchKernelGGL(psh::window_min<0>, mins, block, 0, c.stream, fields_dev, plane, n, w, tiles_dev, after, cprep, min_part);
    hipLaunchKernelGGL(psh::window_min_final, dim3(1), block, 0, c.stream, static_cast<const double *>(min_part),
                       nr_fields * psh::kMinBlocks, prep);
    hipLaunchKernelGGL(psh::window_min<1>, mins, block, 0, c.stream, fields_dev, plane, n, w, tiles_dev, after, cprep, min_part);
    hipLaunchKernelGGL(psh::window_min_final, dim3(1), block, 0, c.stream, static_cast<const double *>(min_part),
                       nr_fields * psh::kMinBlocks, prep + 1);
    hipLaunchKernelGGL(psh::window_min<2>, mins, block, 0, c.stream, fields_dev, plane, n, w, tiles_dev, after, cprep, min_part);
    hipLaunchKernelGGL(psh::window_min_final, dim3(nr_fields), block, 0, c.stream, static_cast<const double *>(min_part),
                       psh::kMinBlocks, prep + 2);
    PSH_HIP(hipGetLastError());
    for (int f = 0; f < nr_fields; ++f) {
      hipLaunchKernelGGL(psh::masked_field, image, block, 0, c.stream, fields_dev, plane, n, w, tiles_dev, after, cprep, f, masked);
      PSH_HIP(hipGetLastError());
      if (int rc = psh_fft_rfft2_dev(masked, m, n, f == 0 ? acc : one)) return rc;
      if (f > 0)
        hipLaunchKernelGGL(psh::spectrum_add, dim3(psh::sweep_blocks(half)), block, 0, c.stream, acc, static_cast<const double2 *>(one),
                           half, f == nr_fields - 1 ? 1.0 / static_cast<double>(nr_fields) : 1.0);
    }
    const double2 *spec = acc;
    hipLaunchKernelGGL(psh::half_partial<false>, dim3(rows), block, 0, c.stream, spec, m, nc, n_even, static_cast<const double *>(stats), partial);
    hipLaunchKernelGGL(psh::half_final<false>, dim3(1), block, 0, c.stream, static_cast<const psh::dd *>(partial), rows, cells, stats);
    hipLaunchKernelGGL(psh::half_partial<true>, dim3(rows), block, 0, c.stream, spec, m, nc, n_even, static_cast<const double *>(stats), partial);
    hipLaunchKernelGGL(psh::half_final<true>, dim3(1), block, 0, c.stream, static_cast<const psh::dd *>(partial), rows, cells, stats);
    hipLaunchKernelGGL(psh::standardise_abs, dim3(psh::sweep_blocks(half)), block, 0, c.stream, spec, half,
                       static_cast<const double *>(stats), planes_dev + static_cast<size_t>(w.plane) * half);
    if (m > 2)
      hipLaunchKernelGGL(psh::symmetrise_columns, dim3((m / 2 + psh::kThreads - 1) / psh::kThreads, 2), block, 0, c.stream,
                         planes_dev + static_cast<size_t>(w.plane) * half, m, nc, n_even);
    PSH_HIP(hipGetLastError());
  }
  return PSH_OK;
}

extern "C" int psh_ssft_merge_dev(double *plane_dev, const double *weights_dev, const double *newfilter_dev, size_t count) {
  PSH_ENTER(c);
  if (!plane_dev || !weights_dev || !newfilter_dev) return fail(PSH_EINVAL, "ssft_merge: NULL pointer");
  if (count == 0) return fail(PSH_EINVAL, "ssft_merge: empty plane");
  hipLaunchKernelGGL(psh::merge, dim3(psh::sweep_blocks(count)), dim3(psh::kThreads), 0, c.stream, plane_dev, weights_dev,
                     newfilter_dev, count);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

extern "C" int psh_ssft_generate_dev(const double *white_dev, int K, int m, int n, const double *planes_dev, int nplanes,
                                     const long long *wins_host, int nwin, const double *tiles_dev, size_t tiles_count,
                                     const double *sM_dev, double *out_dev) {
  PSH_ENTER(c);
  if (!white_dev || !planes_dev || !wins_host || !sM_dev || !out_dev) return fail(PSH_EINVAL, "ssft_generate: NULL pointer");
  if (K < 1 || K > 65535 || nplanes < 1 || nwin < 1) return fail(PSH_EINVAL, "ssft_generate: 1..65535 fields, at least one plane and window");
  if (!psh::shape_ok(m, n))
    return fail(PSH_EUNSUPPORTED, "ssft_generate: (%d,%d) - sides: powers of two up to 8192 or any length up to 4096", m, n);
  std::vector<psh::Win> wins;
  if (int rc = psh::read_windows("ssft_generate", wins_host, nwin, m, n, tiles_count, tiles_dev != nullptr, nplanes, &wins)) return rc;
  const int nc = n / 2 + 1;
  const size_t plane = static_cast<size_t>(m) * n, half = static_cast<size_t>(m) * nc;
  const size_t spec_bytes = half * sizeof(double2), field_bytes = plane * sizeof(double);
  // K spectra of the white noise, the column pass's plane, K filtered fields, K (mean, std) pairs
  psh::Scratch blk;
  if (int rc = blk.alloc((K + 1) * spec_bytes + K * field_bytes + K * sizeof(double2))) return rc;
  char *spectra = blk.as<char>();
  void *colpass = blk.at<void>(K * spec_bytes);
  double2 *stats = blk.at<double2>((K + 1) * spec_bytes);
  double *flN = blk.at<double>((K + 1) * spec_bytes + K * sizeof(double2));
  for (int k = 0; k < K; ++k)
    if (int rc = psh_fft_rfft2_dev(white_dev + static_cast<size_t>(k) * plane, m, n, spectra + k * spec_bytes)) return rc;
  PSH_HIP(hipMemsetAsync(out_dev, 0, K * field_bytes, c.stream));
  const dim3 block(psh::kThreads);
  // planes in the order in which the table first names them, whatever their numbers: a bank that numbers the same
  // planes differently adds every pixel's windows in the same order
  std::vector<char> done(nplanes, 0);
  for (const psh::Win &first : wins) {
    const int p = first.plane;
    if (done[p] || first.i1 <= first.i0 || first.j1 <= first.j0) continue;
    done[p] = 1;
    // the members one after the other against the same plane: it is read from HBM once and stays in the cache for the rest
    for (int k = 0; k < K; ++k)
      if (int rc = psh::fft_irfft2_weighted(spectra + k * spec_bytes, planes_dev + static_cast<size_t>(p) * half, m, n,
                                            flN + static_cast<size_t>(k) * plane, colpass))
        return rc;
    for (const psh::Win &w : wins) {
      if (w.plane != p || w.i1 <= w.i0 || w.j1 <= w.j0) continue;
      hipLaunchKernelGGL(psh::accumulate, dim3((w.j1 - w.j0 + psh::kThreads - 1) / psh::kThreads, w.i1 - w.i0, K), block, 0, c.stream,
                         static_cast<const double *>(flN), plane, n, w, tiles_dev, out_dev);
      PSH_HIP(hipGetLastError());
    }
  }
  const unsigned bx = std::min(psh::sweep_blocks(plane), 1024u);
  hipLaunchKernelGGL(psh::divide_by_masks, dim3(bx, K), block, 0, c.stream, out_dev, plane, sM_dev);
  PSH_HIP(hipGetLastError());
  if (int rc = psh_rainfarm_std_dev(out_dev, K, plane, reinterpret_cast<double *>(stats))) return rc;  // mean, then mean squared deviation
  hipLaunchKernelGGL(psh::standardise, dim3(bx, K), block, 0, c.stream, out_dev, plane, static_cast<const double2 *>(stats));
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}
