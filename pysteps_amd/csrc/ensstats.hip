// Ensemble mean and exceedance probabilities (pysteps/postprocessing/ensemblestats.py mean, excprob) on gfx950: the
// products of a member stack (k, npix), float32 or float64, made where the members lie.
//
// One streaming kernel reads every member once and writes, in the same pass, the mean plane and one probability plane
// per threshold (up to 16; more thresholds are further passes of the caller).  A thread owns 16 bytes of consecutive
// pixels for all k members, so every sum runs in member order exactly as NumPy's axis-0 reduction does:
//   mean, plain         s = 0; s += X[j]; s / k in the accumulator type (the input's own, or float64 for float32
//                       members when the caller asks for it: the reference's float64 block is the widened members)
//   mean, NaN-aware     values < X_thr count as NaN; NaN adds 0 to the sum and nothing to the count; sum / count, 0/0 = NaN
//   excprob             count = #{finite and >= thr}, nfinite = #{finite}; count / k if nfinite == k else NaN, or
//                       count / nfinite (NaN at 0) with ignore_nan; float64, one correctly rounded division
// The sums start from +0.0 like np.add.reduce does (its identity): members that are all -0.0 sum to +0.0, as in NumPy;
// for every other input 0 + X[0] is X[0] bit for bit.  Quotients of float32 accumulators are taken in float64 and rounded once more:
// with 53 >= 2 * 24 + 2 bits this equals the correctly rounded float32 quotient, and it is what np.nanmean does.
// A float32 member is compared with ceil32(thr), the smallest float32 >= thr: x >= thr and x < thr in float64 are
// x >= ceil32(thr) and x < ceil32(thr) in float32, for every float32 x.
//
// No LDS, no atomics, no cross-lane step.  kEnsUnroll member loads are issued before the first is consumed (the member
// stride is npix: nothing else hides HBM latency); thresholds arrive by value (SGPRs), counters live in VGPRs.  Planes
// that are not 16-byte aligned (npix * sizeof(T) % 16 != 0) take the same kernel with one pixel per thread.
// Compulsory traffic: k * npix * sizeof(T) read, (mean + T planes) * npix * 8 written (4 for a float32 mean).
#include <cfloat>

#include "common.h"

namespace psh {
namespace {

constexpr int kEnsThreads = 256;
constexpr int kEnsMaxThr = 16;
constexpr int kEnsUnroll = 8;  // member loads in flight per thread
constexpr int kEnsMaxMembers = 1 << 24;  // float32 holds every count exactly

enum { kMeanNone = 0, kMeanPlain = 1, kMeanNan = 2 };

template <typename T>
struct EnsParams {
  T thr[kEnsMaxThr];  // ceil to T of the thresholds, NaN beyond the call's count
  T mean_thr;         // NaN: no X_thr
  int nthr, k, mean_mode, prob_ignore_nan;
};

template <typename T, int P>
struct alignas(sizeof(T) * P > 16 ? 16 : sizeof(T) * P) Pack {
  T v[P];
};

template <typename T, typename A, int NT, int P>
__global__ __launch_bounds__(kEnsThreads) void ens_products(const T *__restrict__ members, size_t npix, EnsParams<T> prm,
                                                            A *__restrict__ mean_out, double *__restrict__ prob_out) {
  const size_t i = static_cast<size_t>(blockIdx.x) * kEnsThreads + threadIdx.x;
  const size_t p0 = i * P;
  if (p0 >= npix) return;  // npix is a multiple of P: a thread's pixels are all inside or all outside
  const int k = prm.k, mean_mode = prm.mean_mode;

  A sum[P];
  int cnt[NT > 0 ? NT : 1][P], nfin[P], nval[P];
#pragma unroll
  for (int q = 0; q < P; ++q) {
    sum[q] = static_cast<A>(0.0);
    nfin[q] = nval[q] = 0;
#pragma unroll
    for (int t = 0; t < NT; ++t) cnt[t][q] = 0;
  }

  auto consume = [&](const Pack<T, P> &pk) {
#pragma unroll
    for (int q = 0; q < P; ++q) {
      const T x = pk.v[q];
      if (NT > 0) {
        const bool fin = __builtin_isfinite(x);
        nfin[q] += fin ? 1 : 0;
        const T xf = fin ? x : static_cast<T>(NAN);
#pragma unroll
        for (int t = 0; t < NT; ++t) cnt[t][q] += (xf >= prm.thr[t]) ? 1 : 0;
      }
      if (mean_mode == kMeanPlain) {
        sum[q] += static_cast<A>(x);
      } else if (mean_mode == kMeanNan) {
        const bool drop = (x != x) || (x < prm.mean_thr);
        sum[q] += drop ? static_cast<A>(0.0) : static_cast<A>(x);
        nval[q] += drop ? 0 : 1;
      }
    }
  };

  const T *src = members + p0;
  int j = 0;
  for (; j + kEnsUnroll <= k; j += kEnsUnroll) {
    Pack<T, P> pk[kEnsUnroll];
#pragma unroll
    for (int u = 0; u < kEnsUnroll; ++u) pk[u] = *reinterpret_cast<const Pack<T, P> *>(src + static_cast<size_t>(j + u) * npix);
#pragma unroll
    for (int u = 0; u < kEnsUnroll; ++u) consume(pk[u]);
  }
  for (; j < k; ++j) consume(*reinterpret_cast<const Pack<T, P> *>(src + static_cast<size_t>(j) * npix));

  if (mean_mode != kMeanNone) {
    Pack<A, P> m;
#pragma unroll
    for (int q = 0; q < P; ++q) {
      const double den = mean_mode == kMeanPlain ? static_cast<double>(k) : static_cast<double>(nval[q]);
      m.v[q] = static_cast<A>(static_cast<double>(sum[q]) / den);  // 0 / 0 = NaN
    }
    *reinterpret_cast<Pack<A, P> *>(mean_out + p0) = m;
  }
  if (NT > 0) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (t < prm.nthr) {  // uniform: the kernel is instantiated for the next count in {1, 2, 4, 8, 16}
        Pack<double, P> pr;
#pragma unroll
        for (int q = 0; q < P; ++q) {
          const double c = static_cast<double>(cnt[t][q]);
          if (prm.prob_ignore_nan)
            pr.v[q] = nfin[q] > 0 ? c / static_cast<double>(nfin[q]) : static_cast<double>(NAN);
          else
            pr.v[q] = nfin[q] == k ? c / static_cast<double>(k) : static_cast<double>(NAN);
        }
        *reinterpret_cast<Pack<double, P> *>(prob_out + static_cast<size_t>(t) * npix + p0) = pr;
      }
    }
  }
}

// the smallest T >= t (NaN stays NaN; beyond the largest finite T: +inf, which no finite member reaches)
template <typename T>
T ceil_to(double t);
template <>
double ceil_to<double>(double t) {
  return t;
}
template <>
float ceil_to<float>(double t) {
  if (t != t) return NAN;
  if (t > static_cast<double>(FLT_MAX)) return INFINITY;
  if (t < -static_cast<double>(FLT_MAX)) return -FLT_MAX;
  float f = static_cast<float>(t);
  if (static_cast<double>(f) < t) f = nextafterf(f, INFINITY);
  return f;
}

template <typename T, typename A, int NT, int P>
int launch_one(const T *members, size_t npix, const EnsParams<T> &prm, void *mean, double *prob, hipStream_t s) {
  const size_t threads = npix / P, blocks = (threads + kEnsThreads - 1) / kEnsThreads;
  if (blocks > 0xffffffu) return fail(PSH_EUNSUPPORTED, "ens_products: %zu pixels", npix);  // grid x block < 2^32 threads
  hipLaunchKernelGGL((ens_products<T, A, NT, P>), dim3(static_cast<unsigned>(blocks)), dim3(kEnsThreads), 0, s, members, npix,
                     prm, static_cast<A *>(mean), prob);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

template <typename T, typename A, int P>
int launch_nt(const T *members, size_t npix, const EnsParams<T> &prm, void *mean, double *prob, hipStream_t s) {
  const int n = prm.nthr;
  if (n == 0) return launch_one<T, A, 0, P>(members, npix, prm, mean, prob, s);
  if (n == 1) return launch_one<T, A, 1, P>(members, npix, prm, mean, prob, s);
  if (n == 2) return launch_one<T, A, 2, P>(members, npix, prm, mean, prob, s);
  if (n <= 4) return launch_one<T, A, 4, P>(members, npix, prm, mean, prob, s);
  if (n <= 8) return launch_one<T, A, 8, P>(members, npix, prm, mean, prob, s);
  return launch_one<T, A, 16, P>(members, npix, prm, mean, prob, s);
}

template <typename T, typename A>
int run(const void *members_dev, size_t npix, int k, const double *thr, int nthr, int prob_ignore_nan, int mean_mode,
        int mean_has_thr, double mean_thr, void *mean, double *prob, hipStream_t s) {
  EnsParams<T> prm;
  for (int t = 0; t < kEnsMaxThr; ++t) prm.thr[t] = t < nthr ? ceil_to<T>(thr[t]) : static_cast<T>(NAN);
  prm.mean_thr = mean_has_thr ? ceil_to<T>(mean_thr) : static_cast<T>(NAN);
  prm.nthr = nthr;
  prm.k = k;
  prm.mean_mode = mean_mode;
  prm.prob_ignore_nan = prob_ignore_nan;
  const T *members = static_cast<const T *>(members_dev);
  constexpr int P = 16 / sizeof(T);
  // a thread's 16-byte loads and stores need every plane of the stack and of the products aligned
  const bool wide = (npix % P) == 0 && (reinterpret_cast<uintptr_t>(members_dev) % 16) == 0 &&
                    (reinterpret_cast<uintptr_t>(mean) % 16) == 0 && (reinterpret_cast<uintptr_t>(prob) % 16) == 0;
  return wide ? launch_nt<T, A, P>(members, npix, prm, mean, prob, s) : launch_nt<T, A, 1>(members, npix, prm, mean, prob, s);
}

}  // namespace
}  // namespace psh

using psh::fail;

extern "C" int psh_ens_products_dev(const void *members_dev, int members_f64, int k, size_t npix, const double *thresholds_host,
                                    int n_thresholds, int prob_ignore_nan, int mean_ignore_nan, int mean_has_thr,
                                    double mean_thr, int accumulate_f64, void *mean_dev, double *probs_dev) {
  using namespace psh;
  PSH_ENTER(c);
  if (!members_dev) return fail(PSH_EINVAL, "ens_products: NULL member stack");
  if (k < 1 || k > kEnsMaxMembers) return fail(PSH_EINVAL, "ens_products: %d members (1..%d)", k, kEnsMaxMembers);
  if (npix < 1) return fail(PSH_EINVAL, "ens_products: empty planes");
  if (n_thresholds < 0 || n_thresholds > kEnsMaxThr)
    return fail(PSH_EINVAL, "ens_products: %d thresholds in one pass (0..%d)", n_thresholds, kEnsMaxThr);
  if (n_thresholds > 0 && (!thresholds_host || !probs_dev)) return fail(PSH_EINVAL, "ens_products: thresholds without a list or an output");
  if (!probs_dev) n_thresholds = 0;
  if (!mean_dev && n_thresholds == 0) return fail(PSH_EINVAL, "ens_products: no product requested");
  const int mean_mode = !mean_dev ? kMeanNone : (mean_ignore_nan || mean_has_thr) ? kMeanNan : kMeanPlain;
  if (members_f64)
    return run<double, double>(members_dev, npix, k, thresholds_host, n_thresholds, prob_ignore_nan, mean_mode, mean_has_thr,
                               mean_thr, mean_dev, probs_dev, c.stream);
  if (accumulate_f64)
    return run<float, double>(members_dev, npix, k, thresholds_host, n_thresholds, prob_ignore_nan, mean_mode, mean_has_thr,
                              mean_thr, mean_dev, probs_dev, c.stream);
  return run<float, float>(members_dev, npix, k, thresholds_host, n_thresholds, prob_ignore_nan, mean_mode, mean_has_thr,
                           mean_thr, mean_dev, probs_dev, c.stream);
}
