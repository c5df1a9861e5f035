// Windowed aggregation, domain clipping and squaring of resident fields (pysteps/utils/dimension.py): the step of a
// pysteps workflow between the transforms and the scores that changes a field's SHAPE.
//   aggregate_fields        :219-339  reshape to (k, w, P), np.sum / mean / nansum / nanmean over axis 1
//   aggregate_fields_space  :120-216  two such passes, y then x, with a rounding in between
//   aggregate_fields_time   :25-117   one pass along the time axis; here also as a running accumulator
//   clip_domain             :342-451  a rectangle of every plane into a plane filled with zerovalue
//   square_domain           :454-599  the same with the field's minimum (pad) or zeros (inverse of a crop) as fill
//
// The order is the contract.  NumPy reduces a non-innermost axis strictly in index order, starting from the identity +0,
// in the array's own type: ((0 + x0) + x1) + ...; so does every loop here: one thread owns an output element and adds
// its w inputs in index order.  The leading +0 changes one thing only, and NumPy shows it: a window of -0.0 sums to +0.0.
// The nan* methods add +0 in place of a NaN (np.nansum's _replace_nan).  mean / nanmean divide by the window size / the
// count of non-NaN values; NumPy forms that quotient in float64 and stores it in the field's type, and so does
// agg_finish (for float32 this is the correctly rounded float32 quotient: 53 >= 2 * 24 + 2 bits).  Nothing here may contract a multiply with an add or reassociate; there is no
// multiply, and the loops are written out in order.
//
// An array is seen as (pre, len, post) around the aggregated axis.  Two regimes:
//   post >= 2  (time axis, y axis)  aggregate_outer: consecutive threads own consecutive `post` positions, every step of
//              the walk is one coalesced row of loads (16-byte vectors where post and the addresses allow)
//   post == 1  (x axis)  aggregate_inner: the w inputs of an output are contiguous.  A block stages the inputs of 256
//              outputs in LDS, 128 bytes of each output's window at a time, with coalesced loads; thread g then adds the
//              entries of row g in order.  Rows are padded to an odd length so that stride-w reads spread over the banks
// aggregate_space fuses the two passes of an upscale: per tile of one output row the column aggregates (regime 1 walk,
// straight from HBM) are rounded into an LDS row, then one thread per output cell adds its wx entries in order.
#include <algorithm>

#include "common.h"

namespace psh {
namespace {

template <class T, int N> struct alignas(sizeof(T) * N) Pack {
  T e[N];
};

__device__ __forceinline__ bool agg_skips(int method) { return method >= PSH_AGG_NANSUM; }
__device__ __forceinline__ bool agg_divides(int method) { return method == PSH_AGG_MEAN || method == PSH_AGG_NANMEAN; }

// one more input of a window: NaN counts as +0 under the nan* methods and is not counted
template <class T> __device__ __forceinline__ void agg_add(T x, bool skip, T &acc, unsigned &cnt) {
  const bool ok = !skip || x == x;
  acc = acc + (ok ? x : T(0));
  cnt += ok ? 1u : 0u;
}

// cnt is the window size under mean (nothing was skipped) and the number of non-NaN inputs under nanmean: 0 / 0 = NaN
template <class T> __device__ __forceinline__ T agg_finish(T acc, unsigned cnt, bool divide) {
  return divide ? static_cast<T>(static_cast<double>(acc) / static_cast<double>(cnt)) : acc;
}

// ---- post >= 2 ---------------------------------------------------------------------------------------------------------
// N > 1: `post`, `in` and `out` allow 16-byte vectors of N elements; postv = post / N
template <class T, int N>
__global__ __launch_bounds__(256) void aggregate_outer(const T *__restrict__ in, T *__restrict__ out, size_t pre, size_t len,
                                                       size_t postv, size_t K, int w, int method) {
  using P = Pack<T, N>;
  const bool skip = agg_skips(method), divide = agg_divides(method);
  const P *inv = reinterpret_cast<const P *>(in);
  P *outv = reinterpret_cast<P *>(out);
  const size_t total = pre * K * postv;
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t o = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; o < total; o += stride) {
    const size_t p = o % postv, ak = o / postv, k = ak % K, a = ak / K;
    const P *src = inv + (a * len + k * static_cast<size_t>(w)) * postv + p;
    T acc[N];
    unsigned cnt[N];
#pragma unroll
    for (int j = 0; j < N; ++j) acc[j] = T(0), cnt[j] = 0;
    for (int i = 0; i < w; ++i) {
      const P v = src[static_cast<size_t>(i) * postv];
#pragma unroll
      for (int j = 0; j < N; ++j) agg_add(v.e[j], skip, acc[j], cnt[j]);
    }
    P r;
#pragma unroll
    for (int j = 0; j < N; ++j) r.e[j] = agg_finish(acc[j], cnt[j], divide);
    outv[o] = r;
  }
}

// ---- post == 1 ---------------------------------------------------------------------------------------------------------
constexpr int kInnerOutputs = 256;  // outputs (LDS rows) of one tile: one per thread
template <class T> constexpr int inner_chunk() { return 128 / static_cast<int>(sizeof(T)); }  // entries of a row staged at a time

// rows of `len`, K windows of w in each (the last len - K w entries of a row are not read).  VEC (16-byte loads): the
// windows of consecutive outputs are contiguous (len == K w), a whole window fits a chunk, `in` is 16-byte aligned
template <class T, bool VEC>
__global__ __launch_bounds__(256) void aggregate_inner(const T *__restrict__ in, T *__restrict__ out, size_t rows, size_t len,
                                                       size_t K, int w, int method) {
  constexpr int CMAX = inner_chunk<T>();
  constexpr int N = 16 / static_cast<int>(sizeof(T));
  __shared__ T tile[kInnerOutputs * (CMAX + 1)];
  __shared__ size_t base[kInnerOutputs];
  const bool skip = agg_skips(method), divide = agg_divides(method);
  const int tid = threadIdx.x;
  const int C = w < CMAX ? w : CMAX, Cp = C | 1;  // odd row length: thread g reads g * Cp + c, one bank each
  const size_t total = rows * K;
  for (size_t o0 = static_cast<size_t>(blockIdx.x) * kInnerOutputs; o0 < total; o0 += static_cast<size_t>(gridDim.x) * kInnerOutputs) {
    const int G = static_cast<int>(total - o0 < static_cast<size_t>(kInnerOutputs) ? total - o0 : kInnerOutputs);
    if (tid < G) {
      const size_t o = o0 + tid;
      base[tid] = (o / K) * len + (o % K) * static_cast<size_t>(w);
    }
    T acc = T(0);
    unsigned cnt = 0;
    for (int c0 = 0; c0 < w; c0 += C) {
      const int cw = w - c0 < C ? w - c0 : C;
      __syncthreads();  // base[] is written; the previous chunk has been added
      if (VEC) {  // one contiguous span of G * w elements from in + o0 * w (o0 is a multiple of 256: aligned)
        const T *span = in + o0 * static_cast<size_t>(w);
        const int count = G * w, nvec = count / N;
        for (int v = tid; v < nvec; v += kInnerOutputs) {
          const Pack<T, N> p = reinterpret_cast<const Pack<T, N> *>(span)[v];
#pragma unroll
          for (int j = 0; j < N; ++j) {
            const int e = v * N + j, g = e / w;
            tile[g * Cp + (e - g * w)] = p.e[j];
          }
        }
        for (int e = nvec * N + tid; e < count; e += kInnerOutputs) {
          const int g = e / w;
          tile[g * Cp + (e - g * w)] = span[e];
        }
      } else {
        for (int e = tid; e < G * cw; e += kInnerOutputs) {
          const int g = e / cw, c = e - g * cw;
          tile[g * Cp + c] = in[base[g] + c0 + c];
        }
      }
      __syncthreads();
      if (tid < G)
        for (int c = 0; c < cw; ++c) agg_add(tile[tid * Cp + c], skip, acc, cnt);
    }
    if (tid < G) out[o0 + tid] = agg_finish(acc, cnt, divide);
  }
}

// ---- the fused upscale ---------------------------------------------------------------------------------------------------
constexpr int kSpaceCols = 1024;      // input columns of a tile: their aggregates over wy rows live in LDS
constexpr int kSpaceMaxWindow = PSH_SPACE_MAX_WINDOW;  // wy, wx served by the fused kernel: at least 16 outputs per tile

// outputs of a tile: as many as kSpaceCols columns hold, a multiple of 4 so that every tile starts on a vector
__host__ __device__ inline int space_tile_outputs(int wx, int KX) {
  const int fit = (kSpaceCols / wx) & ~3;
  return KX < fit ? KX : fit;
}

// (planes, m, n) -> (planes, m / wy, n / wx); mean or nanmean.  N > 1: n and `in` allow 16-byte vectors of N elements
template <class T, int N>
__global__ __launch_bounds__(256) void aggregate_space(const T *__restrict__ in, T *__restrict__ out, size_t planes, int m, int n,
                                                       int wy, int wx, int skip_nan) {
  __shared__ T col[2 * kSpaceCols];  // TX rows of wx | 1 entries: at most 1024 + 1024 / wx
  const bool skip = skip_nan != 0;
  const int tid = threadIdx.x;
  const int KY = m / wy, KX = n / wx, TX = space_tile_outputs(wx, KX), Cp = wx | 1;
  const int tiles_x = (KX + TX - 1) / TX;
  const size_t tiles = planes * KY * tiles_x;
  for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int tile_x = static_cast<int>(t % tiles_x);
    const size_t row = t / tiles_x;  // plane * KY + oy
    const size_t plane = row / KY, oy = row % KY;
    const int tx0 = tile_x * TX, ntx = KX - tx0 < TX ? KX - tx0 : TX;
    const int ncols = ntx * wx;  // a multiple of N where N > 1: TX wx is one, and so is n
    const T *src = in + (plane * m + oy * wy) * static_cast<size_t>(n) + static_cast<size_t>(tx0) * wx;
    for (int x = tid * N; x < ncols; x += 256 * N) {
      T acc[N];
      unsigned cnt[N];
#pragma unroll
      for (int j = 0; j < N; ++j) acc[j] = T(0), cnt[j] = 0;
      for (int r = 0; r < wy; ++r) {
        const Pack<T, N> v = *reinterpret_cast<const Pack<T, N> *>(src + static_cast<size_t>(r) * n + x);
#pragma unroll
        for (int j = 0; j < N; ++j) agg_add(v.e[j], skip, acc[j], cnt[j]);
      }
#pragma unroll
      for (int j = 0; j < N; ++j) {
        const int g = (x + j) / wx;
        col[g * Cp + (x + j - g * wx)] = agg_finish(acc[j], cnt[j], true);  // rounded in the field's type, as the first pass stores it
      }
    }
    __syncthreads();
    for (int g = tid; g < ntx; g += 256) {
      T acc = T(0);
      unsigned cnt = 0;
      for (int j = 0; j < wx; ++j) agg_add(col[g * Cp + j], skip, acc, cnt);
      out[row * KX + tx0 + g] = agg_finish(acc, cnt, true);
    }
    __syncthreads();  // col[] is free for the next tile
  }
}

// ---- the running accumulator ---------------------------------------------------------------------------------------------
// acc = (first ? 0 : acc) + the input, NaN as +0 and uncounted under the nan* methods; last: the division.  TI widens
// to TA exactly.  N > 1: all buffers allow vectors of N elements
template <class TI, class TA, int N>
__global__ __launch_bounds__(256) void accumulate_step(const TI *__restrict__ in, TA *__restrict__ acc, unsigned *__restrict__ count, size_t nvec,
                                                       int method, int first, int last, unsigned nframes) {
  const bool skip = agg_skips(method), divide = last && agg_divides(method);
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < nvec; i += stride) {
    const Pack<TI, N> x = reinterpret_cast<const Pack<TI, N> *>(in)[i];
    Pack<TA, N> a;
    Pack<unsigned, N> c;
#pragma unroll
    for (int j = 0; j < N; ++j) a.e[j] = TA(0), c.e[j] = 0;
    if (!first) {
      a = reinterpret_cast<const Pack<TA, N> *>(acc)[i];
      if (count) c = reinterpret_cast<const Pack<unsigned, N> *>(count)[i];
    }
#pragma unroll
    for (int j = 0; j < N; ++j) {
      agg_add(static_cast<TA>(x.e[j]), skip, a.e[j], c.e[j]);
      if (divide) a.e[j] = agg_finish(a.e[j], count ? c.e[j] : nframes, true);
    }
    reinterpret_cast<Pack<TA, N> *>(acc)[i] = a;
    if (count) reinterpret_cast<Pack<unsigned, N> *>(count)[i] = c;
  }
}

// ---- rectangle copy --------------------------------------------------------------------------------------------------------
struct WindowArgs {
  size_t planes;
  int in_m, in_n, src_y, src_x;
  int out_m, out_n, dst_y, dst_x;
  int h, w;
  double fill;
};

// every output element: inside the destination rectangle the source element (converted), elsewhere the fill.  N > 1: out_n
// and `out` allow 16-byte vector stores of N elements; the loads are element-wise (the rectangles need not line up)
template <class TI, class TO, int N>
__global__ __launch_bounds__(256) void window_copy(const TI *__restrict__ in, TO *__restrict__ out, WindowArgs a) {
  const size_t rowv = static_cast<size_t>(a.out_n) / N;
  const size_t total = a.planes * a.out_m * rowv;
  const TO fill = static_cast<TO>(a.fill);
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t o = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; o < total; o += stride) {
    const int xv = static_cast<int>(o % rowv);
    const size_t py = o / rowv;
    const int y = static_cast<int>(py % a.out_m);
    const size_t plane = py / a.out_m;
    const int ry = y - a.dst_y;
    const bool row_in = ry >= 0 && ry < a.h;
    const TI *src = in + (plane * a.in_m + (row_in ? a.src_y + ry : 0)) * static_cast<size_t>(a.in_n) + a.src_x;
    Pack<TO, N> r;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const int rx = xv * N + j - a.dst_x;
      r.e[j] = (row_in && rx >= 0 && rx < a.w) ? static_cast<TO>(src[rx]) : fill;
    }
    reinterpret_cast<Pack<TO, N> *>(out)[o] = r;
  }
}

// ---- launchers -------------------------------------------------------------------------------------------------------------
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline unsigned blocks_for(size_t work_items, int cu_count) {
  const size_t want = (work_items + 255) / 256, cap = static_cast<size_t>(cu_count) * 16;
  return static_cast<unsigned>(std::max<size_t>(1, std::min(want, cap)));
}

template <class T> void launch_axis(const Context &c, const T *in, T *out, size_t pre, size_t len, size_t post, int w, int method) {
  constexpr int N = 16 / static_cast<int>(sizeof(T));
  const size_t K = len / w;
  if (post >= 2) {
    if (post % N == 0 && aligned16(in) && aligned16(out))
      hipLaunchKernelGGL((aggregate_outer<T, N>), dim3(blocks_for(pre * K * (post / N), c.cu_count)), dim3(256), 0, c.stream, in, out, pre,
                         len, post / N, K, w, method);
    else
      hipLaunchKernelGGL((aggregate_outer<T, 1>), dim3(blocks_for(pre * K * post, c.cu_count)), dim3(256), 0, c.stream, in, out, pre, len,
                         post, K, w, method);
    return;
  }
  const size_t tiles = (pre * K + kInnerOutputs - 1) / kInnerOutputs;
  const dim3 grid(static_cast<unsigned>(std::max<size_t>(1, std::min(tiles, static_cast<size_t>(c.cu_count) * 8))));
  if (len == K * static_cast<size_t>(w) && w <= inner_chunk<T>() && aligned16(in))
    hipLaunchKernelGGL((aggregate_inner<T, true>), grid, dim3(256), 0, c.stream, in, out, pre, len, K, w, method);
  else
    hipLaunchKernelGGL((aggregate_inner<T, false>), grid, dim3(256), 0, c.stream, in, out, pre, len, K, w, method);
}

template <class T> void launch_space(const Context &c, const T *in, T *out, size_t planes, int m, int n, int wy, int wx, int skip) {
  constexpr int N = 16 / static_cast<int>(sizeof(T));
  const int KX = n / wx, TX = space_tile_outputs(wx, KX);
  const size_t tiles = planes * (m / wy) * ((KX + TX - 1) / TX);
  const dim3 grid(static_cast<unsigned>(std::max<size_t>(1, std::min(tiles, static_cast<size_t>(c.cu_count) * 16))));
  // a vector never straddles a tile: tiles start at multiples of TX wx, a multiple of 4 unless the row is a single tile
  if (n % N == 0 && aligned16(in) && (TX == KX || (TX * wx) % N == 0))
    hipLaunchKernelGGL((aggregate_space<T, N>), grid, dim3(256), 0, c.stream, in, out, planes, m, n, wy, wx, skip);
  else
    hipLaunchKernelGGL((aggregate_space<T, 1>), grid, dim3(256), 0, c.stream, in, out, planes, m, n, wy, wx, skip);
}

template <class TI, class TA> void launch_accumulate(const Context &c, const TI *in, TA *acc, unsigned *count, size_t n, int method, int first,
                                                     int last, unsigned nframes) {
  constexpr int N = 16 / static_cast<int>(sizeof(TI));
  const bool vec = n % N == 0 && aligned16(in) && reinterpret_cast<uintptr_t>(acc) % (sizeof(TA) * N) == 0 &&
                   (!count || reinterpret_cast<uintptr_t>(count) % (sizeof(unsigned) * N) == 0);
  if (vec)
    hipLaunchKernelGGL((accumulate_step<TI, TA, N>), dim3(blocks_for(n / N, c.cu_count)), dim3(256), 0, c.stream, in, acc, count, n / N, method,
                       first, last, nframes);
  else
    hipLaunchKernelGGL((accumulate_step<TI, TA, 1>), dim3(blocks_for(n, c.cu_count)), dim3(256), 0, c.stream, in, acc, count, n, method, first,
                       last, nframes);
}

template <class TI, class TO> void launch_window(const Context &c, const TI *in, TO *out, const WindowArgs &a) {
  constexpr int N = 16 / static_cast<int>(sizeof(TO));
  const size_t total = a.planes * a.out_m * static_cast<size_t>(a.out_n);
  if (a.out_n % N == 0 && aligned16(out))
    hipLaunchKernelGGL((window_copy<TI, TO, N>), dim3(blocks_for(total / N, c.cu_count)), dim3(256), 0, c.stream, in, out, a);
  else
    hipLaunchKernelGGL((window_copy<TI, TO, 1>), dim3(blocks_for(total, c.cu_count)), dim3(256), 0, c.stream, in, out, a);
}

inline bool element_aligned(const void *p, bool f64) { return (reinterpret_cast<uintptr_t>(p) & (f64 ? 7 : 3)) == 0; }
constexpr size_t kMaxExtent = size_t(1) << 30;  // per-tile index arithmetic is 32-bit

}  // namespace
}  // namespace psh

extern "C" int psh_aggregate_axis_dev(const void *in_dev, int is_f64, size_t pre, size_t len, size_t post, int window, int method,
                                      int trim, void *out_dev) {
  PSH_ENTER(c);
  if (method < PSH_AGG_SUM || method > PSH_AGG_NANMEAN) return psh::fail(PSH_EINVAL, "aggregate_axis: unknown method %d", method);
  if (window <= 0 || static_cast<size_t>(window) > psh::kMaxExtent)
    return psh::fail(PSH_EINVAL, "aggregate_axis: window %d out of range", window);
  if (len % window && !trim) return psh::fail(PSH_EINVAL, "aggregate_axis: window %d does not divide %zu", window, len);
  if (pre * (len / window) * post == 0) return PSH_OK;
  if (!in_dev || !out_dev) return psh::fail(PSH_EINVAL, "aggregate_axis: NULL pointer");
  if (!psh::element_aligned(in_dev, is_f64) || !psh::element_aligned(out_dev, is_f64))
    return psh::fail(PSH_EINVAL, "aggregate_axis: buffers must be aligned to their element");
  if (is_f64)
    psh::launch_axis(c, static_cast<const double *>(in_dev), static_cast<double *>(out_dev), pre, len, post, window, method);
  else
    psh::launch_axis(c, static_cast<const float *>(in_dev), static_cast<float *>(out_dev), pre, len, post, window, method);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

extern "C" int psh_aggregate_space_dev(const void *in_dev, int is_f64, size_t planes, int m, int n, int wy, int wx, int ignore_nan,
                                       int route, void *out_dev) {
  PSH_ENTER(c);
  if (m <= 0 || n <= 0 || wy <= 0 || wx <= 0 || static_cast<size_t>(m) > psh::kMaxExtent || static_cast<size_t>(n) > psh::kMaxExtent)
    return psh::fail(PSH_EINVAL, "aggregate_space: bad shape %d x %d, window %d x %d", m, n, wy, wx);
  if (m % wy || n % wx) return psh::fail(PSH_EINVAL, "aggregate_space: window %d x %d does not divide %d x %d", wy, wx, m, n);
  if (route < PSH_SPACE_AUTO || route > PSH_SPACE_TWO_LAUNCH) return psh::fail(PSH_EINVAL, "aggregate_space: unknown route %d", route);
  const bool fits = wy <= psh::kSpaceMaxWindow && wx <= psh::kSpaceMaxWindow;
  if (route == PSH_SPACE_FUSED && !fits)
    return psh::fail(PSH_EINVAL, "aggregate_space: the fused kernel serves windows up to %d x %d", psh::kSpaceMaxWindow, psh::kSpaceMaxWindow);
  if (planes == 0) return PSH_OK;
  if (!in_dev || !out_dev) return psh::fail(PSH_EINVAL, "aggregate_space: NULL pointer");
  if (!psh::element_aligned(in_dev, is_f64) || !psh::element_aligned(out_dev, is_f64))
    return psh::fail(PSH_EINVAL, "aggregate_space: buffers must be aligned to their element");
  const int method = ignore_nan ? PSH_AGG_NANMEAN : PSH_AGG_MEAN;
  if (fits && route != PSH_SPACE_TWO_LAUNCH) {
    if (is_f64)
      psh::launch_space(c, static_cast<const double *>(in_dev), static_cast<double *>(out_dev), planes, m, n, wy, wx, ignore_nan != 0);
    else
      psh::launch_space(c, static_cast<const float *>(in_dev), static_cast<float *>(out_dev), planes, m, n, wy, wx, ignore_nan != 0);
    PSH_HIP(hipGetLastError());
    return PSH_OK;
  }
  // y then x through a plane of column aggregates, exactly the two calls of the reference
  const size_t KY = static_cast<size_t>(m / wy);
  psh::Scratch mid;
  if (int rc = mid.alloc(planes * KY * n * (is_f64 ? 8 : 4))) return rc;
  if (is_f64) {
    psh::launch_axis(c, static_cast<const double *>(in_dev), mid.as<double>(), planes, m, n, wy, method);
    PSH_HIP(hipGetLastError());
    psh::launch_axis(c, mid.as<const double>(), static_cast<double *>(out_dev), planes * KY, n, 1, wx, method);
  } else {
    psh::launch_axis(c, static_cast<const float *>(in_dev), mid.as<float>(), planes, m, n, wy, method);
    PSH_HIP(hipGetLastError());
    psh::launch_axis(c, mid.as<const float>(), static_cast<float *>(out_dev), planes * KY, n, 1, wx, method);
  }
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

extern "C" int psh_accumulate_step_dev(const void *in_dev, int in_f64, void *acc_dev, int acc_f64, unsigned *count_dev, size_t n,
                                       int method, int first, int last, int nframes) {
  PSH_ENTER(c);
  if (method < PSH_AGG_SUM || method > PSH_AGG_NANMEAN) return psh::fail(PSH_EINVAL, "accumulate_step: unknown method %d", method);
  if (in_f64 && !acc_f64) return psh::fail(PSH_EINVAL, "accumulate_step: a float64 input needs a float64 accumulator");
  if (nframes <= 0) return psh::fail(PSH_EINVAL, "accumulate_step: nframes %d", nframes);
  if (method == PSH_AGG_NANMEAN && !count_dev) return psh::fail(PSH_EINVAL, "accumulate_step: nanmean needs the count plane");
  if (method != PSH_AGG_NANMEAN) count_dev = nullptr;
  if (n == 0) return PSH_OK;
  if (!in_dev || !acc_dev) return psh::fail(PSH_EINVAL, "accumulate_step: NULL pointer");
  if (!psh::element_aligned(in_dev, in_f64) || !psh::element_aligned(acc_dev, acc_f64) || !psh::element_aligned(count_dev, false))
    return psh::fail(PSH_EINVAL, "accumulate_step: buffers must be aligned to their element");
  const unsigned nf = static_cast<unsigned>(nframes);
  if (in_f64)
    psh::launch_accumulate(c, static_cast<const double *>(in_dev), static_cast<double *>(acc_dev), count_dev, n, method, first, last, nf);
  else if (acc_f64)
    psh::launch_accumulate(c, static_cast<const float *>(in_dev), static_cast<double *>(acc_dev), count_dev, n, method, first, last, nf);
  else
    psh::launch_accumulate(c, static_cast<const float *>(in_dev), static_cast<float *>(acc_dev), count_dev, n, method, first, last, nf);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

extern "C" int psh_window_copy_dev(const void *in_dev, int in_f64, size_t planes, int in_m, int in_n, int src_y, int src_x,
                                   void *out_dev, int out_f64, int out_m, int out_n, int dst_y, int dst_x, int h, int w, double fill) {
  PSH_ENTER(c);
  if (in_m < 0 || in_n < 0 || out_m < 0 || out_n < 0 || h < 0 || w < 0 || static_cast<size_t>(in_m) > psh::kMaxExtent ||
      static_cast<size_t>(in_n) > psh::kMaxExtent || static_cast<size_t>(out_m) > psh::kMaxExtent || static_cast<size_t>(out_n) > psh::kMaxExtent)
    return psh::fail(PSH_EINVAL, "window_copy: bad shape");
  // the rectangle lies inside both planes (an empty one lies anywhere)
  if (h > 0 && w > 0 &&
      (src_y < 0 || src_x < 0 || dst_y < 0 || dst_x < 0 || src_y > in_m - h || src_x > in_n - w || dst_y > out_m - h || dst_x > out_n - w))
    return psh::fail(PSH_EINVAL, "window_copy: the %d x %d rectangle at (%d, %d) -> (%d, %d) leaves a %d x %d or %d x %d plane", h, w, src_y,
                     src_x, dst_y, dst_x, in_m, in_n, out_m, out_n);
  if (planes * out_m * static_cast<size_t>(out_n) == 0) return PSH_OK;
  if (h == 0 || w == 0) h = w = 0, src_y = src_x = dst_y = dst_x = 0;
  if (!out_dev || (!in_dev && h > 0)) return psh::fail(PSH_EINVAL, "window_copy: NULL pointer");
  if (!psh::element_aligned(in_dev, in_f64) || !psh::element_aligned(out_dev, out_f64))
    return psh::fail(PSH_EINVAL, "window_copy: buffers must be aligned to their element");
  const psh::WindowArgs a{planes, in_m, in_n, src_y, src_x, out_m, out_n, dst_y, dst_x, h, w, fill};
  if (in_f64 && out_f64)
    psh::launch_window(c, static_cast<const double *>(in_dev), static_cast<double *>(out_dev), a);
  else if (in_f64)
    psh::launch_window(c, static_cast<const double *>(in_dev), static_cast<float *>(out_dev), a);
  else if (out_f64)
    psh::launch_window(c, static_cast<const float *>(in_dev), static_cast<double *>(out_dev), a);
  else
    psh::launch_window(c, static_cast<const float *>(in_dev), static_cast<float *>(out_dev), a);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

extern "C" int psh_field_min_dev(const void *in_dev, int is_f64, size_t n, double *min_out) {
  PSH_ENTER(c);
  if (!in_dev || !min_out || n == 0) return psh::fail(PSH_EINVAL, "field_min: NULL pointer or empty field");
  psh::FieldStats st;
  if (int rc = is_f64 ? psh::field_stats_full_f64(static_cast<const double *>(in_dev), n, &st)
                      : psh::field_stats_full(static_cast<const float *>(in_dev), n, &st))
    return rc;
  // np.min: any NaN gives NaN; an infinity is a value
  *min_out = st.nonfinite - st.neg_inf - st.pos_inf > 0 ? NAN : st.nanmin();
  return PSH_OK;
}
