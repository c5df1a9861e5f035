// The DARTS motion estimate (pysteps/motion/darts.py) on gfx950: the spectral band of the frames, the normal
// equations of the least-squares system and the synthesis of the dense field.  The small solve stays on the host.
//
// Reference arithmetic, restated:
//   F = fftn(frames moved to (m, n, T))  - here rfft2 per frame (csrc/fft.hip), then a T-point DFT along time of only
//   the bins the reference reads: k_y in [-K_y, K_y], k_x in [-K_x, K_x] (K = N + M), k_t in [-N_t, N_t], wrapped
//   modulo the side as NumPy's negative indices wrap.  The k_x bins rfft2 does not keep come from Hermitian symmetry.
//   Row i of M = [A | B], (k_t, k_y, k_x) = unravel(i, (2N_t+1, 2N_y+1, 2N_x+1)) - N, column p of A / B with
//   (kp_y, kp_x) = unravel(p, (2M_y+1, 2M_x+1)) - M, i_ = k_y - kp_y, j_ = k_x - kp_x, R_ = F[i_, j_, k_t]:
//     A[i, p] = ((c1 / T_y) * i_) * R_,   B[i, p] = ((c1 / T_x) * j_) * R_,   y[i] = k_t * F[k_y, k_x, k_t]
//   (a real factor times a complex value: NumPy's complex product with a zero imaginary part, i.e. both parts scaled).
//   MM = M^H M and M^H y are reduced without materialising M: per-block partial sums into a slab, then a fixed-order
//   sum over the blocks - no atomics, two runs are bit-identical.
//   The field: Re(ifft2 of a spectrum with at most (2M_y+1)(2M_x+1) non-zero bins) as a direct sum over those bins,
//   phases reduced exactly in integers, (k y) mod m, then sincospi.
#include <algorithm>

#include "common.h"

namespace psh {
namespace {

constexpr int kDartsThreads = 256;
constexpr int kDartsMaxFrames = 64;  // time twiddles travel as a kernel argument
constexpr int kDartsMaxCols = 128;   // columns of M = 2 (2M_y+1)(2M_x+1)
constexpr int kDartsMaxBins = kDartsMaxCols / 2;
constexpr int kGramRows = 8;         // rows of M per LDS chunk
constexpr int kGramAcc = 16;         // outputs per thread and block: kDartsThreads * kGramAcc per output group
constexpr int kGramBlocks = 256;     // row ranges (= slab depth)

struct TimeTwiddles {
  double2 w[kDartsMaxFrames];  // exp(-2 pi i j / T), j < T
};

struct SynthBins {
  int ky[kDartsMaxBins];  // in [0, m)
  int kx[kDartsMaxBins];  // in [0, n)
  double2 v[2][kDartsMaxBins];
};

__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
#pragma clang fp contract(off)
  return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

// conj(a) * b
__device__ __forceinline__ double2 cmulc(double2 a, double2 b) {
#pragma clang fp contract(off)
  return make_double2(a.x * b.x + a.y * b.y, a.x * b.y - a.y * b.x);
}

__device__ __forceinline__ int wrap(int k, int side) {
  const int r = k % side;
  return r < 0 ? r + side : r;
}

template <typename T>
__global__ __launch_bounds__(kDartsThreads) void darts_nonfinite(const T *__restrict__ in, size_t count, int *__restrict__ flag) {
  for (size_t i = static_cast<size_t>(blockIdx.x) * kDartsThreads + threadIdx.x; i < count;
       i += static_cast<size_t>(gridDim.x) * kDartsThreads) {
    if (!isfinite(static_cast<double>(in[i]))) *flag = 1;  // every writer stores the same value
  }
}

// one frame's spectrum (m, n/2+1) -> its (2K_y+1, 2K_x+1) band plane
__global__ __launch_bounds__(kDartsThreads) void darts_gather(const double2 *__restrict__ spec, int m, int n, int ky, int kx,
                                                              double2 *__restrict__ plane) {
  const int by = 2 * ky + 1, bx = 2 * kx + 1;
  const int e = blockIdx.x * kDartsThreads + threadIdx.x;
  if (e >= by * bx) return;
  const int iy = e / bx, ix = e - iy * bx;
  const int yw = wrap(iy - ky, m), xw = wrap(ix - kx, n);
  const int nc = n / 2 + 1;
  double2 v;
  if (xw < nc) {
    v = spec[static_cast<size_t>(yw) * nc + xw];
  } else {
    const int ym = yw == 0 ? 0 : m - yw;
    const double2 s = spec[static_cast<size_t>(ym) * nc + (n - xw)];
    v = make_double2(s.x, -s.y);
  }
  plane[e] = v;
}

// planes (T, P) -> cube (2N_t+1, P): cube[k_t + N_t] = sum_t planes[t] exp(-2 pi i k_t t / T), t ascending
__global__ __launch_bounds__(kDartsThreads) void darts_time_dft(const double2 *__restrict__ planes, int T, int P, int nt,
                                                                TimeTwiddles tw, double2 *__restrict__ cube) {
#pragma clang fp contract(off)
  const int e = blockIdx.x * kDartsThreads + threadIdx.x;
  if (e >= P) return;
  for (int it = 0; it <= 2 * nt; ++it) {
    const int kt = wrap(it - nt, T);
    double2 acc = make_double2(0.0, 0.0);
    for (int t = 0; t < T; ++t) {
      const double2 p = cmul(planes[static_cast<size_t>(t) * P + e], tw.w[(kt * t) % T]);
      acc.x += p.x;
      acc.y += p.y;
    }
    cube[static_cast<size_t>(it) * P + e] = acc;
  }
}

struct GramArgs {
  const double2 *cube;
  int Nt, Ny, Nx, My, Mx;
  int by, bx;     // band plane: 2K_y+1, 2K_x+1
  int rows;       // (2N_t+1)(2N_y+1)(2N_x+1)
  int ncol;       // 2 (2M_y+1)(2M_x+1)
  double cy, cx;  // c1 / T_y, c1 / T_x
};

// entry c of row i of [M | y] (c == ncol: y[i]), the reference's arithmetic
__device__ __forceinline__ double2 row_entry(const GramArgs &a, int i, int c) {
#pragma clang fp contract(off)
  const int wy = 2 * a.Ny + 1, wx = 2 * a.Nx + 1;
  const int it = i / (wy * wx), rem = i - it * (wy * wx);
  const int k_y = rem / wx - a.Ny, k_x = rem % wx - a.Nx;
  const int K_y = (a.by - 1) / 2, K_x = (a.bx - 1) / 2;
  const double2 *plane = a.cube + static_cast<size_t>(it) * a.by * a.bx;
  if (c == a.ncol) {
    const double2 f = plane[(k_y + K_y) * a.bx + (k_x + K_x)];
    const double k_t = static_cast<double>(it - a.Nt);
    return make_double2(k_t * f.x, k_t * f.y);
  }
  const int nb = a.ncol / 2;
  const bool is_b = c >= nb;
  const int p = is_b ? c - nb : c;
  const int wpx = 2 * a.Mx + 1;
  const int kp_y = p / wpx - a.My, kp_x = p % wpx - a.Mx;
  const int i_ = k_y - kp_y, j_ = k_x - kp_x;
  const double2 r = plane[(i_ + K_y) * a.bx + (j_ + K_x)];
  const double c2 = is_b ? a.cx * static_cast<double>(j_) : a.cy * static_cast<double>(i_);
  return make_double2(c2 * r.x, c2 * r.y);
}

// partial sums of conj(M[:, p]) [M | y][:, q] over the block's row range; output e = p (ncol + 1) + q of group
// blockIdx.y; slab[blockIdx.x][e]
__global__ __launch_bounds__(kDartsThreads) void darts_gram_partial(GramArgs a, int rows_per_block, double2 *__restrict__ slab) {
  __shared__ double2 buf[kGramRows][kDartsMaxCols + 1];
  const int w = a.ncol + 1;
  const int nout = a.ncol * w;
  const int r0 = blockIdx.x * rows_per_block, r1 = min(a.rows, r0 + rows_per_block);
  const int e0 = blockIdx.y * kDartsThreads * kGramAcc + threadIdx.x;
  double2 acc[kGramAcc];
  int pp[kGramAcc], qq[kGramAcc];
#pragma unroll
  for (int k = 0; k < kGramAcc; ++k) {
    acc[k] = make_double2(0.0, 0.0);
    const int e = min(e0 + k * kDartsThreads, nout - 1);
    pp[k] = e / w;
    qq[k] = e - pp[k] * w;
  }
  for (int rc = r0; rc < r1; rc += kGramRows) {
    const int nr = min(kGramRows, r1 - rc);
    __syncthreads();
    for (int j = threadIdx.x; j < nr * w; j += kDartsThreads) {
      const int r = j / w, c = j - r * w;
      buf[r][c] = row_entry(a, rc + r, c);
    }
    __syncthreads();
    for (int r = 0; r < nr; ++r) {
#pragma unroll
      for (int k = 0; k < kGramAcc; ++k) {
        const double2 t = cmulc(buf[r][pp[k]], buf[r][qq[k]]);
        acc[k].x += t.x;
        acc[k].y += t.y;
      }
    }
  }
  double2 *out = slab + static_cast<size_t>(blockIdx.x) * nout;
#pragma unroll
  for (int k = 0; k < kGramAcc; ++k) {
    const int e = e0 + k * kDartsThreads;
    if (e < nout) out[e] = acc[k];
  }
}

// sum over the slab's blocks in ascending order
__global__ __launch_bounds__(kDartsThreads) void darts_gram_final(const double2 *__restrict__ slab, int nblocks, int nout,
                                                                  double2 *__restrict__ out) {
#pragma clang fp contract(off)
  const int e = blockIdx.x * kDartsThreads + threadIdx.x;
  if (e >= nout) return;
  double2 s = make_double2(0.0, 0.0);
  for (int b = 0; b < nblocks; ++b) {
    const double2 v = slab[static_cast<size_t>(b) * nout + e];
    s.x += v.x;
    s.y += v.y;
  }
  out[e] = s;
}

// M (rows, ncol) and y (rows), row-major as np.hstack([A, B]) lays M out
__global__ __launch_bounds__(kDartsThreads) void darts_rows(GramArgs a, double2 *__restrict__ M, double2 *__restrict__ y) {
  const size_t w = static_cast<size_t>(a.ncol) + 1, total = static_cast<size_t>(a.rows) * w;
  for (size_t j = static_cast<size_t>(blockIdx.x) * kDartsThreads + threadIdx.x; j < total;
       j += static_cast<size_t>(gridDim.x) * kDartsThreads) {
    const int i = static_cast<int>(j / w), c = static_cast<int>(j - static_cast<size_t>(i) * w);
    const double2 v = row_entry(a, i, c);
    if (c == a.ncol)
      y[i] = v;
    else
      M[static_cast<size_t>(i) * a.ncol + c] = v;
  }
}

// ex[b][x] = exp(2 pi i (kx_b x mod n) / n); py[c][b][y] = v[c][b] exp(2 pi i (ky_b y mod m) / m)
__global__ __launch_bounds__(kDartsThreads) void darts_synth_tables(SynthBins bins, int nb, int m, int n, double2 *__restrict__ ex,
                                                                    double2 *__restrict__ py) {
  const int e = blockIdx.x * kDartsThreads + threadIdx.x;
  const int b = blockIdx.y;
  if (e < n) {
    const long long r = (static_cast<long long>(bins.kx[b]) * e) % n;
    double s, c;
    sincospi(2.0 * static_cast<double>(r) / static_cast<double>(n), &s, &c);
    ex[static_cast<size_t>(b) * n + e] = make_double2(c, s);
  }
  if (e < m) {
    const long long r = (static_cast<long long>(bins.ky[b]) * e) % m;
    double s, c;
    sincospi(2.0 * static_cast<double>(r) / static_cast<double>(m), &s, &c);
    const double2 ph = make_double2(c, s);
    py[(static_cast<size_t>(0) * nb + b) * m + e] = cmul(bins.v[0][b], ph);
    py[(static_cast<size_t>(1) * nb + b) * m + e] = cmul(bins.v[1][b], ph);
  }
}

// out[c][y][x] = Re(sum_b py[c][b][y] ex[b][x]) / (m n), c = 0 (U), 1 (V)
template <typename T>
__global__ __launch_bounds__(kDartsThreads) void darts_synth(const double2 *__restrict__ ex, const double2 *__restrict__ py, int nb,
                                                             int m, int n, double scale, T *__restrict__ out) {
#pragma clang fp contract(off)
  const int x = blockIdx.x * kDartsThreads + threadIdx.x, y = blockIdx.y;
  if (x >= n) return;
  double s0 = 0.0, s1 = 0.0;
  for (int b = 0; b < nb; ++b) {
    const double2 e = ex[static_cast<size_t>(b) * n + x];
    const double2 p0 = py[static_cast<size_t>(b) * m + y], p1 = py[(static_cast<size_t>(nb) + b) * m + y];
    s0 += p0.x * e.x - p0.y * e.y;
    s1 += p1.x * e.x - p1.y * e.y;
  }
  const size_t at = static_cast<size_t>(y) * n + x, plane = static_cast<size_t>(m) * n;
  out[at] = static_cast<T>(s0 * scale);
  out[plane + at] = static_cast<T>(s1 * scale);
}

unsigned blocks_for(size_t count) {
  return static_cast<unsigned>(std::max<size_t>(1, std::min<size_t>((count + kDartsThreads - 1) / kDartsThreads, 16384)));
}

int check_gram(const char *who, int Nt, int Ny, int Nx, int My, int Mx) {
  if (Nt < 0 || Ny < 0 || Nx < 0 || My < 0 || Mx < 0) return fail(PSH_EINVAL, "%s: negative coefficient count", who);
  const long long ncol = 2LL * (2 * My + 1) * (2 * Mx + 1);
  if (ncol > kDartsMaxCols) return fail(PSH_EUNSUPPORTED, "%s: %lld columns (at most %d)", who, ncol, kDartsMaxCols);
  const long long rows = (2LL * Nt + 1) * (2LL * Ny + 1) * (2LL * Nx + 1);
  const long long band = (2LL * (Ny + My) + 1) * (2LL * (Nx + Mx) + 1);
  if (rows > (1LL << 30) || band > (1LL << 26)) return fail(PSH_EUNSUPPORTED, "%s: %lld rows", who, rows);
  return PSH_OK;
}

GramArgs gram_args(const void *cube_dev, int Nt, int Ny, int Nx, int My, int Mx, double cy, double cx) {
  GramArgs a;
  a.cube = static_cast<const double2 *>(cube_dev);
  a.Nt = Nt;
  a.Ny = Ny;
  a.Nx = Nx;
  a.My = My;
  a.Mx = Mx;
  a.by = 2 * (Ny + My) + 1;
  a.bx = 2 * (Nx + Mx) + 1;
  a.rows = (2 * Nt + 1) * (2 * Ny + 1) * (2 * Nx + 1);
  a.ncol = 2 * (2 * My + 1) * (2 * Mx + 1);
  a.cy = cy;
  a.cx = cx;
  return a;
}

}  // namespace
}  // namespace psh

extern "C" int psh_darts_nonfinite_dev(const void *frames_dev, int f32, size_t count, int *flag_host) {
  using namespace psh;
  PSH_ENTER(c);
  if (!frames_dev || !flag_host) return fail(PSH_EINVAL, "darts_nonfinite: NULL pointer");
  psh::Scratch blk;
  if (int rc = blk.alloc(sizeof(int))) return rc;
  int *flag = blk.as<int>();
  PSH_HIP(hipMemsetAsync(flag, 0, sizeof(int), c.stream));
  if (count) {
    with_real(frames_dev, !f32, [&](auto *frames) {
      hipLaunchKernelGGL(darts_nonfinite, dim3(blocks_for(count)), dim3(kDartsThreads), 0, c.stream, frames, count, flag);
    });
    PSH_HIP(hipGetLastError());
  }
  PSH_HIP(hipMemcpyAsync(flag_host, flag, sizeof(int), hipMemcpyDeviceToHost, c.stream));
  PSH_HIP(hipStreamSynchronize(c.stream));
  return PSH_OK;
}

extern "C" int psh_darts_band_dev(const void *frames_dev, int f32, int T, int m, int n, int ky, int kx, int nt, void *cube_dev) {
  using namespace psh;
  PSH_ENTER(c);
  if (!frames_dev || !cube_dev) return fail(PSH_EINVAL, "darts_band: NULL pointer");
  if (T < 1 || T > kDartsMaxFrames) return fail(PSH_EUNSUPPORTED, "darts_band: %d frames (1..%d)", T, kDartsMaxFrames);
  if (m < 2 || n < 2) return fail(PSH_EINVAL, "darts_band: shape %d x %d", m, n);
  if (ky < 0 || kx < 0 || ky >= m || kx >= n || nt < 0 || nt >= T)
    return fail(PSH_EINVAL, "darts_band: band %d x %d x %d outside %d x %d x %d", ky, kx, nt, m, n, T);
  const int by = 2 * ky + 1, bx = 2 * kx + 1;
  if (static_cast<long long>(by) * bx > (1LL << 26)) return fail(PSH_EUNSUPPORTED, "darts_band: band too large");
  const size_t plane = static_cast<size_t>(m) * n, nc = static_cast<size_t>(n / 2 + 1);
  const size_t P = static_cast<size_t>(by) * bx;
  const size_t spec_bytes = static_cast<size_t>(m) * nc * sizeof(double2);
  const size_t wide_bytes = f32 ? plane * sizeof(double) : 0;
  const size_t planes_bytes = static_cast<size_t>(T) * P * sizeof(double2);
  psh::Scratch blk;
  if (int rc = blk.alloc(spec_bytes + wide_bytes + planes_bytes)) return rc;
  double2 *spec = blk.as<double2>();
  double *wide = blk.at<double>(spec_bytes);
  double2 *planes = blk.at<double2>(spec_bytes + wide_bytes);
  for (int t = 0; t < T; ++t) {
    const double *frame;
    if (f32) {
      if (int rc = psh_convert_dev(static_cast<const float *>(frames_dev) + t * plane, wide, plane, 1)) return rc;
      frame = wide;
    } else {
      frame = static_cast<const double *>(frames_dev) + t * plane;
    }
    if (int rc = psh_fft_rfft2_dev(frame, m, n, spec)) return rc;
    hipLaunchKernelGGL(darts_gather, dim3((P + kDartsThreads - 1) / kDartsThreads), dim3(kDartsThreads), 0, c.stream, spec, m, n,
                       ky, kx, planes + t * P);
    PSH_HIP(hipGetLastError());
  }
  TimeTwiddles tw;
  const long double step = -2.0L * 3.14159265358979323846264338327950288L / static_cast<long double>(T);
  for (int j = 0; j < kDartsMaxFrames; ++j) {
    const long double a = step * static_cast<long double>(j < T ? j : 0);
    tw.w[j] = make_double2(static_cast<double>(cosl(a)), static_cast<double>(sinl(a)));
  }
  hipLaunchKernelGGL(darts_time_dft, dim3((P + kDartsThreads - 1) / kDartsThreads), dim3(kDartsThreads), 0, c.stream,
                     static_cast<const double2 *>(planes), T, static_cast<int>(P), nt, tw, static_cast<double2 *>(cube_dev));
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

extern "C" int psh_darts_gram_dev(const void *cube_dev, int Nt, int Ny, int Nx, int My, int Mx, double cy, double cx, void *out_host) {
  using namespace psh;
  PSH_ENTER(c);
  if (!cube_dev || !out_host) return fail(PSH_EINVAL, "darts_gram: NULL pointer");
  if (int rc = check_gram("darts_gram", Nt, Ny, Nx, My, Mx)) return rc;
  const GramArgs a = gram_args(cube_dev, Nt, Ny, Nx, My, Mx, cy, cx);
  const int nout = a.ncol * (a.ncol + 1);
  const int per_group = kDartsThreads * kGramAcc;
  const int groups = (nout + per_group - 1) / per_group;
  const int nblocks = std::min(kGramBlocks, (a.rows + kGramRows - 1) / kGramRows);
  const int rows_per_block = (a.rows + nblocks - 1) / nblocks;
  psh::Scratch blk;
  if (int rc = blk.alloc((static_cast<size_t>(nblocks) + 1) * nout * sizeof(double2))) return rc;
  double2 *slab = blk.as<double2>(), *out = slab + static_cast<size_t>(nblocks) * nout;
  hipLaunchKernelGGL(darts_gram_partial, dim3(nblocks, groups), dim3(kDartsThreads), 0, c.stream, a, rows_per_block, slab);
  PSH_HIP(hipGetLastError());
  hipLaunchKernelGGL(darts_gram_final, dim3((nout + kDartsThreads - 1) / kDartsThreads), dim3(kDartsThreads), 0, c.stream,
                     static_cast<const double2 *>(slab), nblocks, nout, out);
  PSH_HIP(hipGetLastError());
  PSH_HIP(hipMemcpyAsync(out_host, out, static_cast<size_t>(nout) * sizeof(double2), hipMemcpyDeviceToHost, c.stream));
  PSH_HIP(hipStreamSynchronize(c.stream));
  return PSH_OK;
}

extern "C" int psh_darts_rows_dev(const void *cube_dev, int Nt, int Ny, int Nx, int My, int Mx, double cy, double cx, void *M_dev,
                                  void *y_dev) {
  using namespace psh;
  PSH_ENTER(c);
  if (!cube_dev || !M_dev || !y_dev) return fail(PSH_EINVAL, "darts_rows: NULL pointer");
  if (int rc = check_gram("darts_rows", Nt, Ny, Nx, My, Mx)) return rc;
  const GramArgs a = gram_args(cube_dev, Nt, Ny, Nx, My, Mx, cy, cx);
  const size_t total = static_cast<size_t>(a.rows) * (a.ncol + 1);
  hipLaunchKernelGGL(darts_rows, dim3(blocks_for(total)), dim3(kDartsThreads), 0, c.stream, a, static_cast<double2 *>(M_dev),
                     static_cast<double2 *>(y_dev));
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

extern "C" int psh_darts_synth_dev(const int *ky_host, const int *kx_host, const void *values_host, int nb, int m, int n, int f32,
                                   void *out_dev) {
  using namespace psh;
  PSH_ENTER(c);
  if (!ky_host || !kx_host || !values_host || !out_dev) return fail(PSH_EINVAL, "darts_synth: NULL pointer");
  if (nb < 1 || nb > kDartsMaxBins) return fail(PSH_EUNSUPPORTED, "darts_synth: %d bins (1..%d)", nb, kDartsMaxBins);
  if (m < 1 || n < 1 || m > 65535) return fail(PSH_EINVAL, "darts_synth: shape %d x %d", m, n);
  SynthBins bins = {};
  const double2 *vals = static_cast<const double2 *>(values_host);
  for (int b = 0; b < nb; ++b) {
    if (ky_host[b] < 0 || ky_host[b] >= m || kx_host[b] < 0 || kx_host[b] >= n)
      return fail(PSH_EINVAL, "darts_synth: bin (%d, %d) outside %d x %d", ky_host[b], kx_host[b], m, n);
    bins.ky[b] = ky_host[b];
    bins.kx[b] = kx_host[b];
    bins.v[0][b] = vals[b];
    bins.v[1][b] = vals[nb + b];
  }
  psh::Scratch blk;
  if (int rc = blk.alloc(static_cast<size_t>(nb) * (n + 2 * static_cast<size_t>(m)) * sizeof(double2))) return rc;
  double2 *ex = blk.as<double2>(), *py = ex + static_cast<size_t>(nb) * n;
  const int side = std::max(m, n);
  hipLaunchKernelGGL(darts_synth_tables, dim3((side + kDartsThreads - 1) / kDartsThreads, nb), dim3(kDartsThreads), 0, c.stream,
                     bins, nb, m, n, ex, py);
  PSH_HIP(hipGetLastError());
  const dim3 grid((n + kDartsThreads - 1) / kDartsThreads, m);
  const double scale = 1.0 / (static_cast<double>(m) * static_cast<double>(n));
  with_real(out_dev, !f32, [&](auto *out) {
    hipLaunchKernelGGL(darts_synth, grid, dim3(kDartsThreads), 0, c.stream, static_cast<const double2 *>(ex),
                       static_cast<const double2 *>(py), nb, m, n, scale, out);
  });
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}
