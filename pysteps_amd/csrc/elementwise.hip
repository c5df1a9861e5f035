// Element-wise passes either side of the advection path, kept on the device so that a
// nowcast chain (rain rate -> dB -> LK -> extrapolation -> rain rate) never leaves HBM:
//   dB transform  pysteps/utils/transformation.py:150-232 (dB_transform, forward and inverse)
//   field statistics (min / max over finite values, count of non-finite values) that the
//   reference gets from NumPy scans: nowcasts/extrapolation.py:76 (allow_nonfinite_values),
//   semilagrangian.py:171-172 (outval="min").
// HBM-streaming, dwordx4 where the size allows; NaN stays NaN like in NumPy.
#include <algorithm>
#include <cmath>

#include "common.h"

namespace psh {
namespace {

// the `<` of both directions runs in double against the number NumPy would compare with: a Python float or a
// numpy.float32 meets a float32 field in float32, a numpy.float64 scalar in float64; the caller rounds the threshold
// accordingly (device._compared_as) and the float32 value widens exactly, so one comparison serves both
__device__ __forceinline__ float to_db(float r, double thr, float zerovalue) {
  // R[~(R < thr)] = 10 log10(R); R[R < thr] = zerovalue  (NaN compares false -> log10(NaN) = NaN)
  return static_cast<double>(r) < thr ? zerovalue : 10.0f * log10f(r);
}
__device__ __forceinline__ float from_db(float r, double thr_lin, float zerovalue) {
  const float v = exp10f(r / 10.0f);
  return static_cast<double>(v) < thr_lin ? zerovalue : v;
}

// VEC: dwordx4 body and a scalar tail (both buffers 16-byte aligned); otherwise one element per thread with the same
// arithmetic, for planes that start off alignment (view(k) of a stack whose planes are not a multiple of four pixels)
template <bool INVERSE, bool VEC>
__global__ __launch_bounds__(256) void db_transform(const float *__restrict__ in,
                                                    float *__restrict__ out, size_t n, double thr,
                                                    float zerovalue) {
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  const size_t first = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const size_t n4 = VEC ? n / 4 : 0;
  if (VEC) {
    const float4 *in4 = reinterpret_cast<const float4 *>(in);
    float4 *out4 = reinterpret_cast<float4 *>(out);
    for (size_t i = first; i < n4; i += stride) {
      float4 v = in4[i];
      v.x = INVERSE ? from_db(v.x, thr, zerovalue) : to_db(v.x, thr, zerovalue);
      v.y = INVERSE ? from_db(v.y, thr, zerovalue) : to_db(v.y, thr, zerovalue);
      v.z = INVERSE ? from_db(v.z, thr, zerovalue) : to_db(v.z, thr, zerovalue);
      v.w = INVERSE ? from_db(v.w, thr, zerovalue) : to_db(v.w, thr, zerovalue);
      out4[i] = v;
    }
  }
  for (size_t i = n4 * 4 + first; i < n; i += stride)
    out[i] = INVERSE ? from_db(in[i], thr, zerovalue) : to_db(in[i], thr, zerovalue);
}

// ---- Box-Cox, square root, Z-R laws (transformation.py:27-147, 329-380; conversion.py:96, 262) -------------------------
// Every value is evaluated in double from the input and rounded once at the store; a `<` that decides on a computed value
// (the inverse Box-Cox) compares the STORED value, widened, with the number NumPy would compare with.
struct TransformArgs {
  double p0, p1;  // Box-Cox: Lambda; Z-R: zr_a and the exponent (1 / zr_b towards the rain rate, zr_b towards Z)
  double thr, zerovalue;
};

template <class T, int OP> __device__ __forceinline__ T transform_one(T x, const TransformArgs &a) {
#pragma clang fp contract(off)  // Lambda * R + 1 is two roundings in the reference, and in both loops here
  const double xd = static_cast<double>(x);
  if (OP == PSH_TRANSFORM_BOXCOX) {
    // zeros = R < threshold, decided on the input; log for Lambda == 0, else (R ** Lambda - 1) / Lambda
    if (xd < a.thr) return static_cast<T>(a.zerovalue);
    return static_cast<T>(a.p0 == 0.0 ? log(xd) : (pow(xd, a.p0) - 1.0) / a.p0);
  }
  if (OP == PSH_TRANSFORM_BOXCOX_INVERSE) {
    const T v = static_cast<T>(a.p0 == 0.0 ? exp(xd) : exp(log(a.p0 * xd + 1.0) / a.p0));
    return static_cast<double>(v) < a.thr ? static_cast<T>(a.zerovalue) : v;  // NaN compares false and stays
  }
  if (OP == PSH_TRANSFORM_SQRT) return static_cast<T>(sqrt(xd));
  if (OP == PSH_TRANSFORM_SQUARE) return static_cast<T>(xd * xd);
  if (OP == PSH_TRANSFORM_Z_TO_RATE) return static_cast<T>(pow(xd / a.p0, a.p1));
  return static_cast<T>(a.p0 * pow(xd, a.p1));  // PSH_TRANSFORM_RATE_TO_Z
}

template <class T> struct Vec16;
template <> struct Vec16<float> { using type = float4; };
template <> struct Vec16<double> { using type = double2; };

// VEC: 16-byte vectors and a scalar tail (both buffers 16-byte aligned); otherwise one element per thread, same arithmetic
template <class T, int OP, bool VEC>
__global__ __launch_bounds__(256) void transform_elements(const T *__restrict__ in, T *__restrict__ out, size_t n, TransformArgs a) {
  using V = typename Vec16<T>::type;
  constexpr size_t kPer = 16 / sizeof(T);
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  const size_t first = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const size_t nvec = VEC ? n / kPer : 0;
  if (VEC) {
    const V *inv = reinterpret_cast<const V *>(in);
    V *outv = reinterpret_cast<V *>(out);
    for (size_t i = first; i < nvec; i += stride) {
      V v = inv[i];
      T *e = reinterpret_cast<T *>(&v);
#pragma unroll
      for (size_t j = 0; j < kPer; ++j) e[j] = transform_one<T, OP>(e[j], a);
      outv[i] = v;
    }
  }
  for (size_t i = nvec * kPer + first; i < n; i += stride) out[i] = transform_one<T, OP>(in[i], a);
}

template <class T, int OP> void launch_transform(const T *in, T *out, size_t n, const TransformArgs &a, bool vec, dim3 grid, hipStream_t s) {
  if (vec)
    hipLaunchKernelGGL((transform_elements<T, OP, true>), grid, dim3(256), 0, s, in, out, n, a);
  else
    hipLaunchKernelGGL((transform_elements<T, OP, false>), grid, dim3(256), 0, s, in, out, n, a);
}

template <class T> int launch_transform_op(int op, const T *in, T *out, size_t n, const TransformArgs &a, bool vec, dim3 grid, hipStream_t s) {
  switch (op) {
    case PSH_TRANSFORM_BOXCOX: launch_transform<T, PSH_TRANSFORM_BOXCOX>(in, out, n, a, vec, grid, s); break;
    case PSH_TRANSFORM_BOXCOX_INVERSE: launch_transform<T, PSH_TRANSFORM_BOXCOX_INVERSE>(in, out, n, a, vec, grid, s); break;
    case PSH_TRANSFORM_SQRT: launch_transform<T, PSH_TRANSFORM_SQRT>(in, out, n, a, vec, grid, s); break;
    case PSH_TRANSFORM_SQUARE: launch_transform<T, PSH_TRANSFORM_SQUARE>(in, out, n, a, vec, grid, s); break;
    case PSH_TRANSFORM_Z_TO_RATE: launch_transform<T, PSH_TRANSFORM_Z_TO_RATE>(in, out, n, a, vec, grid, s); break;
    case PSH_TRANSFORM_RATE_TO_Z: launch_transform<T, PSH_TRANSFORM_RATE_TO_Z>(in, out, n, a, vec, grid, s); break;
    default: return fail(PSH_EINVAL, "field_transform: unknown operation %d", op);
  }
  return PSH_OK;
}

constexpr int kStatFields = 5;

// float64 twin of field_stats (double partials): the host path checks float64 inputs BEFORE they are
// narrowed to float32 - a finite value beyond the float32 range must not read as "non-finite input"
__global__ __launch_bounds__(256) void field_stats_f64(const double *__restrict__ in, size_t n,
                                                       double *__restrict__ partial) {
  double mn = INFINITY, mx = -INFINITY, bad = 0.0, ninf = 0.0, pinf = 0.0;
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
    const double v = in[i];
    if (isfinite(v)) {
      mn = fmin(mn, v);
      mx = fmax(mx, v);
    } else {
      bad += 1.0;
      ninf += v == -INFINITY ? 1.0 : 0.0;
      pinf += v == INFINITY ? 1.0 : 0.0;
    }
  }
  __shared__ double s[kStatFields][4];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    mn = fmin(mn, __shfl_xor(mn, d));
    mx = fmax(mx, __shfl_xor(mx, d));
    bad += __shfl_xor(bad, d);
    ninf += __shfl_xor(ninf, d);
    pinf += __shfl_xor(pinf, d);
  }
  if ((threadIdx.x & 63) == 0) {
    s[0][threadIdx.x >> 6] = mn;
    s[1][threadIdx.x >> 6] = mx;
    s[2][threadIdx.x >> 6] = bad;
    s[3][threadIdx.x >> 6] = ninf;
    s[4][threadIdx.x >> 6] = pinf;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double *o = partial + kStatFields * blockIdx.x;
    o[0] = fmin(fmin(s[0][0], s[0][1]), fmin(s[0][2], s[0][3]));
    o[1] = fmax(fmax(s[1][0], s[1][1]), fmax(s[1][2], s[1][3]));
    for (int k = 2; k < kStatFields; ++k) o[k] = s[k][0] + s[k][1] + s[k][2] + s[k][3];
  }
}

__global__ __launch_bounds__(256) void field_stats(const float *__restrict__ in, size_t n,
                                                   float *__restrict__ partial) {
  // per block: min / max over finite values, counts of non-finite values, of -inf and of +inf
  // (counts < 2^24 per block: exact in float)
  float mn = INFINITY, mx = -INFINITY, bad = 0.f, ninf = 0.f, pinf = 0.f;
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float v = in[i];
    if (isfinite(v)) {
      mn = fminf(mn, v);
      mx = fmaxf(mx, v);
    } else {
      bad += 1.f;
      ninf += v == -INFINITY ? 1.f : 0.f;
      pinf += v == INFINITY ? 1.f : 0.f;
    }
  }
  __shared__ float s[kStatFields][4];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, d));
    mx = fmaxf(mx, __shfl_xor(mx, d));
    bad += __shfl_xor(bad, d);
    ninf += __shfl_xor(ninf, d);
    pinf += __shfl_xor(pinf, d);
  }
  if ((threadIdx.x & 63) == 0) {
    s[0][threadIdx.x >> 6] = mn;
    s[1][threadIdx.x >> 6] = mx;
    s[2][threadIdx.x >> 6] = bad;
    s[3][threadIdx.x >> 6] = ninf;
    s[4][threadIdx.x >> 6] = pinf;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float *o = partial + kStatFields * blockIdx.x;
    o[0] = fminf(fminf(s[0][0], s[0][1]), fminf(s[0][2], s[0][3]));
    o[1] = fmaxf(fmaxf(s[1][0], s[1][1]), fmaxf(s[1][2], s[1][3]));
    for (int k = 2; k < kStatFields; ++k) o[k] = s[k][0] + s[k][1] + s[k][2] + s[k][3];
  }
}

// number of elements > thr (NaN compares false, like NumPy): the rain-pixel count of
// pysteps/utils/check_norain.py:48-49
// the comparison runs in double: the caller decides what the threshold is rounded to first (NumPy
// compares a float32 array with a Python float in float32, with a numpy.float64 scalar in float64)
__global__ __launch_bounds__(256) void count_above(const float *__restrict__ in, size_t n, double thr,
                                                   unsigned long long *__restrict__ total) {
  unsigned cnt = 0;
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride)
    cnt += static_cast<double>(in[i]) > thr ? 1u : 0u;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d);
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(total, static_cast<unsigned long long>(cnt));  // integer: order-free
}

template <typename Tin, typename Tout>
__global__ __launch_bounds__(256) void convert_elements(const Tin *__restrict__ in, Tout *__restrict__ out, size_t n) {
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x * 4;
  for (size_t i = (static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 3 < n) {
      Tin v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = in[i + j];
#pragma unroll
      for (int j = 0; j < 4; ++j) out[i + j] = static_cast<Tout>(v[j]);
    } else {
      for (size_t k = i; k < n; ++k) out[k] = static_cast<Tout>(in[k]);
    }
  }
}

}  // namespace
}  // namespace psh

extern "C" int psh_db_transform_dev(const float *in_dev, float *out_dev, size_t n, double threshold,
                                    double zerovalue, int inverse) {
  PSH_ENTER(c);
  if (n == 0) return PSH_OK;
  if (!in_dev || !out_dev) return psh::fail(PSH_EINVAL, "db_transform: NULL pointer");
  if ((reinterpret_cast<uintptr_t>(in_dev) | reinterpret_cast<uintptr_t>(out_dev)) & 3)
    return psh::fail(PSH_EINVAL, "db_transform: buffers must be 4-byte aligned");
  const bool vec = ((reinterpret_cast<uintptr_t>(in_dev) | reinterpret_cast<uintptr_t>(out_dev)) & 15) == 0;
  const dim3 grid(c.cu_count * 8), block(256);
  // threshold: the number each value is compared with, in the units of the values compared (forward: of R; inverse:
  // linear, of 10^(R/10) - transformation.py:227-228), already rounded the way NumPy would round it
  const float zv = static_cast<float>(zerovalue);
  auto kernel = inverse ? (vec ? psh::db_transform<true, true> : psh::db_transform<true, false>)
                        : (vec ? psh::db_transform<false, true> : psh::db_transform<false, false>);
  hipLaunchKernelGGL(kernel, grid, block, 0, c.stream, in_dev, out_dev, n, threshold, zv);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

extern "C" int psh_field_transform_dev(const void *in_dev, void *out_dev, int f32, size_t n, int op, double p0, double p1,
                                       double threshold, double zerovalue) {
  PSH_ENTER(c);
  if (n == 0) return PSH_OK;
  if (!in_dev || !out_dev) return psh::fail(PSH_EINVAL, "field_transform: NULL pointer");
  const uintptr_t both = reinterpret_cast<uintptr_t>(in_dev) | reinterpret_cast<uintptr_t>(out_dev);
  if (both & (f32 ? 3 : 7)) return psh::fail(PSH_EINVAL, "field_transform: buffers must be aligned to their element");
  const bool vec = (both & 15) == 0;
  const dim3 grid(c.cu_count * 8);
  const psh::TransformArgs a{p0, p1, threshold, zerovalue};
  const int rc = f32 ? psh::launch_transform_op(op, static_cast<const float *>(in_dev), static_cast<float *>(out_dev), n, a, vec, grid, c.stream)
                     : psh::launch_transform_op(op, static_cast<const double *>(in_dev), static_cast<double *>(out_dev), n, a, vec, grid, c.stream);
  if (rc) return rc;
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

namespace psh {

hipError_t launch_convert_f64_f32(const double *in, float *out, size_t n, hipStream_t stream) {
  const unsigned grid = static_cast<unsigned>(std::min<size_t>((n / 4 + 255) / 256 + 1, 65535));
  hipLaunchKernelGGL((convert_elements<double, float>), dim3(grid), dim3(256), 0, stream, in, out, n);
  return hipGetLastError();
}

hipError_t launch_convert_f32_f64(const float *in, double *out, size_t n, hipStream_t stream) {
  const unsigned grid = static_cast<unsigned>(std::min<size_t>((n / 4 + 255) / 256 + 1, 65535));
  hipLaunchKernelGGL((convert_elements<float, double>), dim3(grid), dim3(256), 0, stream, in, out, n);
  return hipGetLastError();
}

// synchronous: waits for the library stream
int field_stats_full(const float *in_dev, size_t n, FieldStats *st) {
  Context &c = ctx();
  constexpr int kBlocks = 1024;
  psh::Scratch blk;
  if (int rc = blk.alloc(kStatFields * kBlocks * sizeof(float))) return rc;
  static thread_local float h[kStatFields * kBlocks];
  hipLaunchKernelGGL(field_stats, dim3(kBlocks), dim3(256), 0, c.stream, in_dev, n, blk.as<float>());
  PSH_HIP(hipGetLastError());
  PSH_HIP(hipMemcpyAsync(h, blk.as<float>(), sizeof(h), hipMemcpyDeviceToHost, c.stream));
  PSH_HIP(hipStreamSynchronize(c.stream));
  FieldStats r;
  for (int b = 0; b < kBlocks; ++b) {
    const float *o = h + kStatFields * b;
    r.min_finite = fmin(r.min_finite, o[0]);
    r.max_finite = fmax(r.max_finite, o[1]);
    r.nonfinite += o[2];
    r.neg_inf += o[3];
    r.pos_inf += o[4];
  }
  r.count = static_cast<double>(n);
  *st = r;
  return PSH_OK;
}

int field_stats_full_f64(const double *in_dev, size_t n, FieldStats *st) {
  Context &c = ctx();
  constexpr int kBlocks = 1024;
  psh::Scratch blk;
  if (int rc = blk.alloc(kStatFields * kBlocks * sizeof(double))) return rc;
  static thread_local double h[kStatFields * kBlocks];
  hipLaunchKernelGGL(field_stats_f64, dim3(kBlocks), dim3(256), 0, c.stream, in_dev, n, blk.as<double>());
  PSH_HIP(hipGetLastError());
  PSH_HIP(hipMemcpyAsync(h, blk.as<double>(), sizeof(h), hipMemcpyDeviceToHost, c.stream));
  PSH_HIP(hipStreamSynchronize(c.stream));
  FieldStats r;
  for (int b = 0; b < kBlocks; ++b) {
    const double *o = h + kStatFields * b;
    r.min_finite = fmin(r.min_finite, o[0]);
    r.max_finite = fmax(r.max_finite, o[1]);
    r.nonfinite += o[2];
    r.neg_inf += o[3];
    r.pos_inf += o[4];
  }
  r.count = static_cast<double>(n);
  *st = r;
  return PSH_OK;
}

}  // namespace psh

extern "C" int psh_nonfinite_count_f64_dev(const double *in_dev, size_t n, double *count_out) {
  PSH_ENTER(c);
  if ((!in_dev && n) || !count_out) return psh::fail(PSH_EINVAL, "nonfinite_count: NULL pointer");
  psh::FieldStats st;
  if (int rc = psh::field_stats_full_f64(in_dev, n, &st)) return rc;
  *count_out = st.nonfinite;
  return PSH_OK;
}

extern "C" int psh_count_above_dev(const float *in_dev, size_t n, double threshold, double *count_out,
                                   double *nanmin_out) {
  PSH_ENTER(c);
  if ((!in_dev && n) || !count_out) return psh::fail(PSH_EINVAL, "count_above: NULL pointer");
  psh::FieldStats st;
  if (int rc = psh::field_stats_full(in_dev, n, &st)) return rc;
  const double lowest = st.nanmin();
  if (nanmin_out) *nanmin_out = lowest;
  // threshold NaN = "use the minimum of the field" (precip_thr=None, check_norain.py:46-47)
  const double thr = threshold != threshold ? lowest : threshold;
  psh::Scratch blk;
  if (int rc = blk.alloc(sizeof(unsigned long long))) return rc;
  unsigned long long *count = blk.as<unsigned long long>(), h = 0;
  PSH_HIP(hipMemsetAsync(count, 0, sizeof(unsigned long long), c.stream));
  hipLaunchKernelGGL(psh::count_above, dim3(c.cu_count * 8), dim3(256), 0, c.stream, in_dev, n, thr, count);
  PSH_HIP(hipGetLastError());
  PSH_HIP(hipMemcpyAsync(&h, count, sizeof(h), hipMemcpyDeviceToHost, c.stream));
  PSH_HIP(hipStreamSynchronize(c.stream));
  *count_out = static_cast<double>(h);
  return PSH_OK;
}

namespace psh {
namespace {
__global__ __launch_bounds__(256) void axpy_f64(double *__restrict__ dst, const double *__restrict__ src, double alpha, size_t n) {
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] += alpha * src[i];
}
}  // namespace
}  // namespace psh

extern "C" int psh_axpy_f64_dev(double *dst_dev, const double *src_dev, double alpha, size_t n) {
  PSH_ENTER(c);
  if (n == 0) return PSH_OK;
  if (!dst_dev || !src_dev) return psh::fail(PSH_EINVAL, "axpy: NULL pointer");
  const unsigned blocks = static_cast<unsigned>(std::min<size_t>((n + 255) / 256, static_cast<size_t>(c.cu_count) * 16));
  hipLaunchKernelGGL(psh::axpy_f64, dim3(blocks), dim3(256), 0, c.stream, dst_dev, src_dev, alpha, n);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

extern "C" int psh_convert_dev(const void *in_dev, void *out_dev, size_t n, int to_f64) {
  PSH_ENTER(c);
  if (n == 0) return PSH_OK;
  if (!in_dev || !out_dev) return psh::fail(PSH_EINVAL, "convert: NULL pointer");
  if (to_f64)
    PSH_HIP(psh::launch_convert_f32_f64(static_cast<const float *>(in_dev), static_cast<double *>(out_dev), n, c.stream));
  else
    PSH_HIP(psh::launch_convert_f64_f32(static_cast<const double *>(in_dev), static_cast<float *>(out_dev), n, c.stream));
  return PSH_OK;
}

extern "C" int psh_field_stats_dev(const float *in_dev, size_t n, double *min_out, double *max_out,
                                   double *nonfinite_out, double *nanmin_out) {
  PSH_ENTER(c);
  if (!in_dev && n) return psh::fail(PSH_EINVAL, "field_stats: NULL pointer");
  psh::FieldStats st;
  if (int rc = psh::field_stats_full(in_dev, n, &st)) return rc;
  if (min_out) *min_out = st.min_finite;   // +inf if there is no finite value
  if (max_out) *max_out = st.max_finite;   // -inf if there is no finite value
  if (nonfinite_out) *nonfinite_out = st.nonfinite;
  if (nanmin_out) *nanmin_out = st.nanmin();  // np.nanmin: an infinity is a value, NaN if there is none at all
  return PSH_OK;
}
