// Normal-quantile transform on the device (pysteps/utils/transformation.py:237-326, NQ_transform).
//
//  * forward: the reference evaluates np.interp(x, sort(x), ndtri(pp)) with pp[k] = ((k + 1) - a) / ((n + 1) - 2 a) over the
//    n values that are not NaN.  np.interp places a value at the LAST element of its run of ties, so a pixel's result is
//    ndtri((c - a) / ((n + 1) - 2 a)) with c the number of values <= it, itself included.
//  * psh_nqt_count_le_dev: order-preserving integer keys (-0.0 folded onto 0.0, every NaN on the all-ones key, which no
//    number has and which therefore sorts behind every value), the key-only radix sort of radix_sort.h, and per pixel an
//    upper-bound binary search into the sorted keys.  A run of ties of any length is one search result; there is no
//    limit on it.  The sorted keys go back to values: they are the y table of the inverse.
//  * ndtri: the three-branch rational approximation of Cephes (ndtri.c) in its written order, float64, contraction off.
//  * inverse: scipy.interpolate.interp1d(kind="linear") on one-dimensional float64 tables, which SciPy hands to np.interp:
//    the interval Rqn[j] <= x < Rqn[j + 1] by binary search, a knot returns its value itself, elsewhere
//    slope * (x - x_lo) + y_lo with each operation rounded on its own; the fill values outside the table.
//  * the reductions (smallest result above 0, smallest result, smallest result above that) are integer atomicMin on
//    order-preserving keys: the same bits in every run.
#include "common.h"
#include "radix_sort.h"

#pragma clang fp contract(off)

namespace psh {
namespace {

constexpr int kMaxGridX = 2048;
inline unsigned grid_x(size_t n) { return static_cast<unsigned>(std::min<size_t>((n + kThreads - 1) / kThreads, kMaxGridX)); }

template <class T> struct KeyOf { using type = unsigned long long; };
template <> struct KeyOf<float> { using type = unsigned; };

__device__ __forceinline__ float key_value(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

template <class T> __device__ __forceinline__ typename KeyOf<T>::type nqt_key(T x) {
  using Key = typename KeyOf<T>::type;
  return x != x ? ~Key(0) : okey(x);
}

__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(v, d);
    v = o < v ? o : v;
  }
  return v;
}

template <class T> __global__ __launch_bounds__(kThreads) void nqt_keys(const T *x, size_t n, typename KeyOf<T>::type *keys,
                                                                         unsigned long long *nan_count) {
  unsigned nans = 0;
  const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) {
    const T v = x[i];
    keys[i] = nqt_key(v);
    nans += v != v ? 1u : 0u;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) nans += __shfl_xor(nans, d);
  if ((threadIdx.x & 63) == 0 && nans) atomicAdd(nan_count, static_cast<unsigned long long>(nans));  // integer: order-free
}

// count[i] = number of sorted keys <= the pixel's key among the first nv (the values that are not NaN); 0 for a NaN
template <class T> __global__ __launch_bounds__(kThreads) void nqt_count_le(const T *x, size_t n, const typename KeyOf<T>::type *sorted,
                                                                             size_t nv, unsigned *count) {
  using Key = typename KeyOf<T>::type;
  const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) {
    const T v = x[i];
    unsigned c = 0;
    if (v == v) {
      const Key key = okey(v);
      size_t lo = 0, hi = nv;  // first position whose key is > key
      while (lo < hi) {
        const size_t mid = lo + ((hi - lo) >> 1);
        if (sorted[mid] <= key)
          lo = mid + 1;
        else
          hi = mid;
      }
      c = static_cast<unsigned>(lo);
    }
    count[i] = c;
  }
}

template <class T> __global__ __launch_bounds__(kThreads) void nqt_values(const typename KeyOf<T>::type *sorted, size_t n, size_t nv, T *values) {
  const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride)
    values[i] = i < nv ? static_cast<T>(key_value(sorted[i])) : static_cast<T>(NAN);
}

// ---- ndtri (Cephes ndtri.c) -----------------------------------------------------------------------------------------
__device__ __forceinline__ double polevl(double x, const double *coef, int N) {
  double ans = coef[0];
  for (int i = 1; i <= N; ++i) ans = ans * x + coef[i];
  return ans;
}
__device__ __forceinline__ double p1evl(double x, const double *coef, int N) {
  double ans = x + coef[0];
  for (int i = 1; i < N; ++i) ans = ans * x + coef[i];
  return ans;
}

__device__ double ndtri(double y0) {
  // approximation for 0 <= |y - 0.5| <= 3/8
  const double P0[5] = {-5.99633501014107895267E1, 9.80010754185999661536E1, -5.66762857469070293439E1,
                        1.39312609387279679503E1, -1.23916583867381258016E0};
  const double Q0[8] = {1.95448858338141759834E0, 4.67627912898881538453E0, 8.63602421390890590575E1,
                        -2.25462687854119370527E2, 2.00260212380060660359E2, -8.20372256168333339912E1,
                        1.59056225126211695515E1, -1.18331621121330003142E0};
  // approximation for the interval z = sqrt(-2 log y) between 2 and 8, i.e. y between exp(-2) and exp(-32)
  const double P1[9] = {4.05544892305962419923E0, 3.15251094599893866154E1, 5.71628192246421288162E1,
                        4.40805073893200834700E1, 1.46849561928858024014E1, 2.18663306850790267539E0,
                        -1.40256079171354495875E-1, -3.50424626827848203418E-2, -8.57456785154685413611E-4};
  const double Q1[8] = {1.57799883256466749731E1, 4.53907635128879210584E1, 4.13172038254672030440E1,
                        1.50425385692907503408E1, 2.50464946208309415979E0, -1.42182922854787788574E-1,
                        -3.80806407691578277194E-2, -9.33259480895457427372E-4};
  // approximation for the interval z = sqrt(-2 log y) between 8 and 64
  const double P2[9] = {3.23774891776946035970E0, 6.91522889068984211695E0, 3.93881025292474443415E0,
                        1.33303460815807542389E0, 2.01485389549179081538E-1, 1.23716634817820021358E-2,
                        3.01581553508235416007E-4, 2.65806974686737550832E-6, 6.23974539184983293730E-9};
  const double Q2[8] = {6.02427039364742014255E0, 3.67983563856160859403E0, 1.37702099489081330271E0,
                        2.16236993594496635890E-1, 1.34204006088543189037E-2, 3.28014464682127739104E-4,
                        2.89247864745380683936E-6, 6.79019408009981274425E-9};
  const double s2pi = 2.50662827463100050242E0;
  if (y0 == 0.0) return -INFINITY;
  if (y0 == 1.0) return INFINITY;
  if (!(y0 > 0.0 && y0 < 1.0)) return NAN;
  bool negate = true;
  double y = y0;
  if (y > 1.0 - 0.13533528323661269189) {  // 0.135... = exp(-2)
    y = 1.0 - y;
    negate = false;
  }
  if (y > 0.13533528323661269189) {
    y = y - 0.5;
    const double y2 = y * y;
    double x = y + y * (y2 * polevl(y2, P0, 4) / p1evl(y2, Q0, 8));
    x = x * s2pi;
    return x;
  }
  double x = sqrt(-2.0 * log(y));
  const double x0 = x - log(x) / x;
  const double z = 1.0 / x;
  double x1;
  if (x < 8.0)
    x1 = z * polevl(z, P1, 8) / p1evl(z, Q1, 8);
  else
    x1 = z * polevl(z, P2, 8) / p1evl(z, Q2, 8);
  x = x0 - x1;
  return negate ? -x : x;
}

// plotting position of the c-th smallest value, in the reference's order: ((k + 1) - a) / ((n + 1) - 2 a); den from the host
__device__ __forceinline__ double quantile_of(double c, double a, double den) { return ndtri((c - a) / den); }

// smallest[0]: key of the smallest stored result > 0
template <class Tin, class Tout>
__global__ __launch_bounds__(kThreads) void nqt_forward(const Tin *x, const unsigned *count, size_t n, double a, double den, double zerovalue,
                                                        Tout *out, unsigned long long *smallest) {
  unsigned long long best = ~0ull;
  const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) {
    const Tin v = x[i];
    Tout r = static_cast<Tout>(NAN);
    if (v == v) {
      r = static_cast<double>(v) == zerovalue ? Tout(0) : static_cast<Tout>(quantile_of(static_cast<double>(count[i]), a, den));
      if (r > Tout(0)) {
        const unsigned long long k = okey(static_cast<double>(r));
        best = k < best ? k : best;
      }
    }
    out[i] = r;
  }
  best = wave_min(best);
  if ((threadIdx.x & 63) == 0 && best != ~0ull) atomicMin(smallest, best);
}

__global__ __launch_bounds__(kThreads) void nqt_table(size_t nv, double a, double den, double *rqn) {
  const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
  for (size_t k = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; k < nv; k += stride)
    rqn[k] = quantile_of(static_cast<double>(k + 1), a, den);
}

// smallest[0]: key of the smallest stored result
template <class Tin, class Ty, class Tout>
__global__ __launch_bounds__(kThreads) void nqt_inverse(const Tin *x, size_t n, const double *rqn, const Ty *ys, size_t nt, Tout *out,
                                                        unsigned long long *smallest) {
  unsigned long long best = ~0ull;
  const double x_first = rqn[0], x_last = rqn[nt - 1];
  const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) {
    const Tin v = x[i];
    Tout r = static_cast<Tout>(NAN);
    if (v == v) {
      const double xn = static_cast<double>(v);
      double y;
      if (xn < x_first) {
        y = static_cast<double>(ys[0]);
      } else if (xn > x_last) {
        y = static_cast<double>(ys[nt - 1]);
      } else {
        size_t lo = 0, hi = nt;  // first position whose entry is > xn; x_first <= xn, so it is at least 1
        while (lo < hi) {
          const size_t mid = lo + ((hi - lo) >> 1);
          if (rqn[mid] <= xn)
            lo = mid + 1;
          else
            hi = mid;
        }
        const size_t j = lo - 1;  // rqn[j] <= xn < rqn[j + 1], or the last entry
        const double x_lo = rqn[j], y_lo = static_cast<double>(ys[j]);
        if (j == nt - 1 || x_lo == xn) {
          y = y_lo;  // a knot returns its value itself
        } else {
          const double x_hi = rqn[j + 1], y_hi = static_cast<double>(ys[j + 1]);
          const double slope = (y_hi - y_lo) / (x_hi - x_lo);
          y = slope * (xn - x_lo) + y_lo;
          if (y != y) {  // NaN from one end (an overflowing slope): np.interp tries the other
            y = slope * (xn - x_hi) + y_hi;
            if (y != y && y_lo == y_hi) y = y_lo;
          }
        }
      }
      r = static_cast<Tout>(y);
      if (r == r) {
        const unsigned long long k = okey(static_cast<double>(r));
        best = k < best ? k : best;
      }
    }
    out[i] = r;
  }
  best = wave_min(best);
  if ((threadIdx.x & 63) == 0 && best != ~0ull) atomicMin(smallest, best);
}

// smallest[1]: key of the smallest value above the one of smallest[0]
template <class T> __global__ __launch_bounds__(kThreads) void nqt_above_min(const T *x, size_t n, unsigned long long *smallest) {
  const unsigned long long floor_key = smallest[0];
  unsigned long long best = ~0ull;
  const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) {
    const T v = x[i];
    if (v == v) {
      const unsigned long long k = okey(static_cast<double>(v));
      if (k > floor_key && k < best) best = k;
    }
  }
  best = wave_min(best);
  if ((threadIdx.x & 63) == 0 && best != ~0ull) atomicMin(smallest + 1, best);
}

inline double host_key_value(unsigned long long k) {
  if (k == ~0ull) return NAN;  // nothing qualified
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double d;
  static_assert(sizeof(d) == sizeof(b), "");
  __builtin_memcpy(&d, &b, sizeof(d));
  return d;
}

// device time between four marks on the stream, for a caller that asks for it (stage_ms != NULL)
struct StageMarks {
  hipEvent_t ev[4] = {};
  int used = 0;
  bool on = false;
  ~StageMarks() {
    for (auto &e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  int start(bool want) {
    on = want;
    if (!on) return PSH_OK;
    for (auto &e : ev) PSH_HIP(hipEventCreate(&e));
    return PSH_OK;
  }
  int mark(hipStream_t s) {
    if (on && used < 4) PSH_HIP(hipEventRecord(ev[used++], s));
    return PSH_OK;
  }
  int finish(float *ms) {  // ms[0..2]: between consecutive marks
    if (!on) return PSH_OK;
    if (used != 4) return fail(PSH_EHIP, "nqt_count_le: stage timing failed");
    PSH_HIP(hipEventSynchronize(ev[3]));
    for (int j = 0; j < 3; ++j) PSH_HIP(hipEventElapsedTime(&ms[j], ev[j], ev[j + 1]));
    return PSH_OK;
  }
};

template <class T>
int count_le_impl(const T *x, size_t n, unsigned *count, T *sorted_out, size_t *n_valid, double *min_out, double *max_out, float *stage_ms,
                  hipStream_t s) {
  using Key = typename KeyOf<T>::type;
  constexpr int D = sizeof(Key);
  const Tiling tl = tiling(n);
  const size_t key_bytes = align_up(n * sizeof(Key), 256);
  const size_t ghist_bytes = D * 256 * sizeof(unsigned);
  const size_t table_bytes = static_cast<size_t>(256) * kMaxTiles * sizeof(unsigned);
  Scratch ws;
  if (int rc = ws.alloc(3 * key_bytes + ghist_bytes + table_bytes + 256)) return rc;
  Key *keys = ws.at<Key>(0);
  Key *buf[2] = {ws.at<Key>(key_bytes), ws.at<Key>(2 * key_bytes)};
  unsigned *ghist = ws.at<unsigned>(3 * key_bytes);
  unsigned *table = ws.at<unsigned>(3 * key_bytes + ghist_bytes);
  unsigned long long *nan_count = ws.at<unsigned long long>(3 * key_bytes + ghist_bytes + table_bytes);
  StageMarks marks;
  if (int rc = marks.start(stage_ms != nullptr)) return rc;
  PSH_HIP(hipMemsetAsync(ghist, 0, ghist_bytes, s));
  if (int rc = marks.mark(s)) return rc;
  PSH_HIP(hipMemsetAsync(nan_count, 0, sizeof(unsigned long long), s));
  hipLaunchKernelGGL(nqt_keys<T>, dim3(grid_x(n)), dim3(kThreads), 0, s, x, n, keys, nan_count);
  hipLaunchKernelGGL(hist_all<Key>, dim3(tl.tiles), dim3(kThreads), 0, s, static_cast<const Key *>(keys), n, tl.per, ghist);
  PSH_HIP(hipGetLastError());
  unsigned ghist_host[D * 256];
  unsigned long long nans = 0;
  PSH_HIP(hipMemcpyAsync(ghist_host, ghist, ghist_bytes, hipMemcpyDeviceToHost, s));
  PSH_HIP(hipMemcpyAsync(&nans, nan_count, sizeof(nans), hipMemcpyDeviceToHost, s));
  PSH_HIP(hipStreamSynchronize(s));
  const size_t nv = n - static_cast<size_t>(nans);
  if (int rc = marks.mark(s)) return rc;
  const Key *src = keys;
  int next = 0;
  for (int d = 0; d < D; ++d) {
    bool constant = false;  // a digit that every key shares leaves the order as it is
    for (int j = 0; j < 256; ++j) constant = constant || ghist_host[d * 256 + j] == n;
    if (constant) continue;
    Key *dst = buf[next];
    hipLaunchKernelGGL(pass_count<Key>, dim3(tl.tiles), dim3(kThreads), 0, s, src, n, tl.per, 8 * d, table);
    hipLaunchKernelGGL(pass_scan, dim3(256), dim3(kThreads), 0, s, table, tl.tiles, static_cast<const unsigned *>(ghist + d * 256));
    hipLaunchKernelGGL(pass_scatter<Key>, dim3(tl.tiles), dim3(kThreads), 0, s, src, dst, n, tl.per, 8 * d, static_cast<const unsigned *>(table));
    src = dst;
    next ^= 1;
  }
  if (int rc = marks.mark(s)) return rc;
  hipLaunchKernelGGL(nqt_count_le<T>, dim3(grid_x(n)), dim3(kThreads), 0, s, x, n, src, nv, count);
  hipLaunchKernelGGL(nqt_values<T>, dim3(grid_x(n)), dim3(kThreads), 0, s, src, n, nv, sorted_out);
  PSH_HIP(hipGetLastError());
  if (int rc = marks.mark(s)) return rc;
  T ends[2] = {static_cast<T>(NAN), static_cast<T>(NAN)};
  if (nv) {
    PSH_HIP(hipMemcpyAsync(&ends[0], sorted_out, sizeof(T), hipMemcpyDeviceToHost, s));
    PSH_HIP(hipMemcpyAsync(&ends[1], sorted_out + (nv - 1), sizeof(T), hipMemcpyDeviceToHost, s));
  }
  PSH_HIP(hipStreamSynchronize(s));  // also: the scratch is read until here
  if (int rc = marks.finish(stage_ms)) return rc;
  *n_valid = nv;
  if (min_out) *min_out = static_cast<double>(ends[0]);
  if (max_out) *max_out = static_cast<double>(ends[1]);
  return PSH_OK;
}

// two keys of device scratch, cleared to "nothing qualified"; read back after the caller's launches
struct Smallest {
  Scratch blk;
  int start(hipStream_t s) {
    if (int rc = blk.alloc(2 * sizeof(unsigned long long))) return rc;
    PSH_HIP(hipMemsetAsync(blk.as<void>(), 0xff, 2 * sizeof(unsigned long long), s));
    return PSH_OK;
  }
  unsigned long long *dev() const { return blk.as<unsigned long long>(); }
  int finish(hipStream_t s, double *first, double *second) {
    unsigned long long h[2];
    PSH_HIP(hipMemcpyAsync(h, dev(), sizeof(h), hipMemcpyDeviceToHost, s));
    PSH_HIP(hipStreamSynchronize(s));
    if (first) *first = host_key_value(h[0]);
    if (second) *second = host_key_value(h[1]);
    return PSH_OK;
  }
};

}  // namespace
}  // namespace psh

using psh::fail;

namespace {
constexpr size_t kNqtMaxValues = 0xffffffffull;  // counts and sort positions are uint32
bool misaligned(const void *p, bool f32) { return reinterpret_cast<uintptr_t>(p) & (f32 ? 3 : 7); }
}  // namespace

extern "C" int psh_nqt_count_le_dev(const void *x_dev, int f32, size_t n, unsigned *count_dev, void *sorted_dev, size_t *n_valid,
                                    double *min_out, double *max_out, float *stage_ms) {
  PSH_ENTER(c);
  if (!x_dev || !count_dev || !sorted_dev || !n_valid) return fail(PSH_EINVAL, "nqt_count_le: NULL pointer");
  if (n == 0) return fail(PSH_EINVAL, "nqt_count_le: nothing to count");
  if (n > kNqtMaxValues) return fail(PSH_EUNSUPPORTED, "nqt_count_le: more than 2^32 - 1 values");
  if (misaligned(x_dev, f32) || misaligned(sorted_dev, f32)) return fail(PSH_EINVAL, "nqt_count_le: buffers must be aligned to their element");
  if (f32)
    return psh::count_le_impl(static_cast<const float *>(x_dev), n, count_dev, static_cast<float *>(sorted_dev), n_valid, min_out, max_out, stage_ms, c.stream);
  return psh::count_le_impl(static_cast<const double *>(x_dev), n, count_dev, static_cast<double *>(sorted_dev), n_valid, min_out, max_out, stage_ms,
                            c.stream);
}

extern "C" int psh_nqt_forward_dev(const void *x_dev, int f32, const unsigned *count_dev, size_t n, size_t n_valid, double a, double zerovalue,
                                   void *out_dev, int out_f32, double *threshold_out) {
  PSH_ENTER(c);
  if (!x_dev || !count_dev || !out_dev) return fail(PSH_EINVAL, "nqt_forward: NULL pointer");
  if (n == 0 || n_valid > n || n > kNqtMaxValues) return fail(PSH_EINVAL, "nqt_forward: 1 ... 2^32 - 1 values, n_valid <= n");
  if (misaligned(x_dev, f32) || misaligned(out_dev, out_f32)) return fail(PSH_EINVAL, "nqt_forward: buffers must be aligned to their element");
  psh::Smallest sm;
  if (int rc = sm.start(c.stream)) return rc;
  const double den = static_cast<double>(n_valid + 1) - 2.0 * a;  // (n + 1 - 2 * a) of transformation.py:299
  const dim3 grid(psh::grid_x(n)), block(psh::kThreads);
  psh::with_real(x_dev, !f32, [&](auto *x) {
    psh::with_real(out_dev, !out_f32, [&](auto *out) {
      using Tin = std::remove_const_t<std::remove_pointer_t<decltype(x)>>;
      using Tout = std::remove_pointer_t<decltype(out)>;
      hipLaunchKernelGGL((psh::nqt_forward<Tin, Tout>), grid, block, 0, c.stream, x, count_dev, n, a, den, zerovalue, out, sm.dev());
      return 0;
    });
    return 0;
  });
  PSH_HIP(hipGetLastError());
  return sm.finish(c.stream, threshold_out, nullptr);
}

extern "C" int psh_nqt_table_dev(size_t n_valid, double a, double *rqn_dev) {
  PSH_ENTER(c);
  if (!rqn_dev) return fail(PSH_EINVAL, "nqt_table: NULL pointer");
  if (n_valid == 0 || n_valid > kNqtMaxValues) return fail(PSH_EINVAL, "nqt_table: 1 ... 2^32 - 1 entries");
  const double den = static_cast<double>(n_valid + 1) - 2.0 * a;
  hipLaunchKernelGGL(psh::nqt_table, dim3(psh::grid_x(n_valid)), dim3(psh::kThreads), 0, c.stream, n_valid, a, den, rqn_dev);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

extern "C" int psh_nqt_inverse_dev(const void *x_dev, int f32, size_t n, const double *rqn_dev, const void *sorted_dev, int sorted_f32,
                                   size_t n_table, void *out_dev, int out_f32, double *min_out, double *above_min_out) {
  PSH_ENTER(c);
  if (!x_dev || !rqn_dev || !sorted_dev || !out_dev) return fail(PSH_EINVAL, "nqt_inverse: NULL pointer");
  if (n == 0) return fail(PSH_EINVAL, "nqt_inverse: nothing to transform");
  if (n_table < 2) return fail(PSH_EINVAL, "nqt_inverse: the table needs two entries");
  if (misaligned(x_dev, f32) || misaligned(sorted_dev, sorted_f32) || misaligned(out_dev, out_f32) || misaligned(rqn_dev, false))
    return fail(PSH_EINVAL, "nqt_inverse: buffers must be aligned to their element");
  psh::Smallest sm;
  if (int rc = sm.start(c.stream)) return rc;
  const dim3 grid(psh::grid_x(n)), block(psh::kThreads);
  psh::with_real(x_dev, !f32, [&](auto *x) {
    psh::with_real(sorted_dev, !sorted_f32, [&](auto *ys) {
      psh::with_real(out_dev, !out_f32, [&](auto *out) {
        using Tin = std::remove_const_t<std::remove_pointer_t<decltype(x)>>;
        using Ty = std::remove_const_t<std::remove_pointer_t<decltype(ys)>>;
        using Tout = std::remove_pointer_t<decltype(out)>;
        hipLaunchKernelGGL((psh::nqt_inverse<Tin, Ty, Tout>), grid, block, 0, c.stream, x, n, rqn_dev, ys, n_table, out, sm.dev());
        hipLaunchKernelGGL(psh::nqt_above_min<Tout>, grid, block, 0, c.stream, static_cast<const Tout *>(out), n, sm.dev());
        return 0;
      });
      return 0;
    });
    return 0;
  });
  PSH_HIP(hipGetLastError());
  return sm.finish(c.stream, min_out, above_min_out);
}
