// Deterministic verification on gfx950: the contingency counts of pysteps/verification/detcatscores.py
// (det_cat_fct_accum) and the sums behind the continuous scores of pysteps/verification/detcontscores.py
// (det_cont_fct_accum), for a stack of K forecasts of npix pixels against one observation or a stack of them, float32
// or float64 each on its own.  One read of every member and of its observation.
//
//   detcat_count    a thread walks the member in chunks of four consecutive pixels, chunk c of the member always going
//                   to thread c % (threads of the row of workgroups), and keeps 32-bit counters of hits, misses and
//                   false alarms for up to 8 thresholds; they are widened to 64 bits at the wave reduction, added over
//                   the workgroup through LDS and over the grid by integer atomics (integer adds commute).  pred > thr
//                   and obs > thr with NaN comparing false, as in the reference: a NaN pixel is "no event" on its side.
//   detcat_finish   correct negatives = npix - hits - misses - false alarms.
//   detcont_partial the same walk; per thread the counts of finite observations, finite predictions and finite pairs
//                   and eleven sums as double-double pairs (dd.h): over the pairs res = pred - obs, res^2, |res|,
//                   (pred + obs)^2, obs, pred, obs pred; over each field's finite pixels the value and its square.
//                   res and pred + obs are rounded float64 operations on the widened inputs, their squares and the
//                   product are then added without a further rounding (fma).  Reduced over the wave by shuffles of
//                   (hi, lo), over the workgroup through LDS in wave order; one partial per workgroup.
//   detcont_finish  one wave per member adds the partials in a fixed order.  No floating-point atomics anywhere.
// The chunk -> thread mapping and the grid depend on npix alone, not on K or on where a member lies, so a member's
// sums are the same bits in every run, in every split of a stack into calls and at every alignment: a chunk is read
// by 16-byte loads when its address allows (a member's base is not 16-byte aligned when npix % 4 != 0 for float32 or
// npix is odd for float64) and element by element otherwise and at the member's ragged end.
#include "common.h"
#include "dd.h"
#include "detsums.h"

namespace psh {
namespace {

constexpr int kDetThrBlock = 8;     // thresholds per pass of detcat_count
constexpr int kDetSums = 11;
constexpr int kDetCounts = 4;       // finite observations, finite predictions, finite pairs, +-inf values seen

enum { kSumObs = kPairSums, kSumObs2, kSumPred, kSumPred2 };  // after the pair sums of detsums.h: each field's own

struct DetThresholds {
  double f[kDetThrBlock], o[kDetThrBlock];
  int count;
};

// grid (groups, K); out points at (member 0, first threshold of this pass), out_stride = nthr * 4 words per member
template <typename TF, typename TO>
__global__ __launch_bounds__(kDetThreads) void detcat_count(const TF *__restrict__ fct, const TO *__restrict__ obs, int obs_shared,
                                                             size_t npix, DetThresholds thr, unsigned long long *__restrict__ out,
                                                             size_t out_stride) {
  __shared__ unsigned long long red[kDetThreads / 64][kDetThrBlock * 3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const TF *f = fct + static_cast<size_t>(blockIdx.y) * npix;
  const TO *o = obs + (obs_shared ? 0 : static_cast<size_t>(blockIdx.y) * npix);
  const bool vec_f = aligned16(f), vec_o = aligned16(o);
  unsigned hits[kDetThrBlock], miss[kDetThrBlock], fa[kDetThrBlock];
#pragma unroll
  for (int j = 0; j < kDetThrBlock; ++j) hits[j] = miss[j] = fa[j] = 0u;

  const size_t nchunk = (npix + 3) / 4, stride = static_cast<size_t>(gridDim.x) * kDetThreads;
  for (size_t c = static_cast<size_t>(blockIdx.x) * kDetThreads + tid; c < nchunk; c += stride) {
    double p[4], q[4];
    load4(f, c * 4, npix, vec_f, p);
    load4(o, c * 4, npix, vec_o, q);
#pragma unroll
    for (int j = 0; j < kDetThrBlock; ++j) {
      if (j < thr.count) {  // uniform
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool pb = p[e] > thr.f[j], ob = q[e] > thr.o[j];  // NaN: false
          hits[j] += (pb && ob) ? 1u : 0u;
          miss[j] += (!pb && ob) ? 1u : 0u;
          fa[j] += (pb && !ob) ? 1u : 0u;
        }
      }
    }
  }

#pragma unroll
  for (int j = 0; j < kDetThrBlock; ++j) {
    unsigned long long v[3] = {hits[j], miss[j], fa[j]};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) v[c] += __shfl_down(v[c], d, 64);
      if (lane == 0) red[wave][j * 3 + c] = v[c];
    }
  }
  __syncthreads();
  if (tid < thr.count * 3) {
    unsigned long long v = 0ull;
#pragma unroll
    for (int w = 0; w < kDetThreads / 64; ++w) v += red[w][tid];
    if (v) atomicAdd(out + blockIdx.y * out_stride + (tid / 3) * 4 + tid % 3, v);
  }
}

__global__ void detcat_finish(unsigned long long *__restrict__ out, size_t tables, unsigned long long npix) {
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= tables) return;
  unsigned long long *t = out + i * 4;
  t[3] = npix - t[0] - t[1] - t[2];
}

struct DetPartial {
  dd sum[kDetSums];
  unsigned long long count[kDetCounts];
};

// grid (groups, K); partial[member][group]
template <typename TF, typename TO>
__global__ __launch_bounds__(kDetThreads) void detcont_partial(const TF *__restrict__ fct, const TO *__restrict__ obs, int obs_shared,
                                                                size_t npix, int conditioning, double thr_f, double thr_o,
                                                                DetPartial *__restrict__ partial) {
#pragma clang fp contract(off)
  __shared__ DetPartial s_part[kDetThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const TF *f = fct + static_cast<size_t>(blockIdx.y) * npix;
  const TO *o = obs + (obs_shared ? 0 : static_cast<size_t>(blockIdx.y) * npix);
  const bool vec_f = aligned16(f), vec_o = aligned16(o);
  dd acc[kDetSums];
#pragma unroll
  for (int s = 0; s < kDetSums; ++s) acc[s] = {0.0, 0.0};
  unsigned cnt[kDetCounts] = {0u, 0u, 0u, 0u};

  const size_t nchunk = (npix + 3) / 4, stride = static_cast<size_t>(gridDim.x) * kDetThreads;
  for (size_t c = static_cast<size_t>(blockIdx.x) * kDetThreads + tid; c < nchunk; c += stride) {
    double p[4], q[4];
    load4(f, c * 4, npix, vec_f, p);
    load4(o, c * 4, npix, vec_o, q);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      double pv = p[e], ov = q[e];
      cnt[3] += (__builtin_isinf(pv) ? 1u : 0u) + (__builtin_isinf(ov) ? 1u : 0u);
      if (conditioning) {  // uniform; the excluded pixels become NaN on both sides
        const bool pb = pv > thr_f, ob = ov > thr_o;
        if (!(conditioning == 1 ? (pb || ob) : (pb && ob))) pv = ov = quiet_nan();
      }
      const bool fin_o = __builtin_isfinite(ov), fin_p = __builtin_isfinite(pv);
      if (fin_o) {
        cnt[0] += 1u;
        acc[kSumObs] = dd_add_d(acc[kSumObs], ov);
        acc[kSumObs2] = dd_add_sq(acc[kSumObs2], ov);
      }
      if (fin_p) {
        cnt[1] += 1u;
        acc[kSumPred] = dd_add_d(acc[kSumPred], pv);
        acc[kSumPred2] = dd_add_sq(acc[kSumPred2], pv);
      }
      const double res = pv - ov, both = pv + ov;
      if (fin_o && fin_p && __builtin_isfinite(res)) {  // the reference counts the pairs whose residual is finite
        cnt[2] += 1u;
        acc[kSumRes] = dd_add_d(acc[kSumRes], res);
        acc[kSumRes2] = dd_add_sq(acc[kSumRes2], res);
        acc[kSumAbs] = dd_add_d(acc[kSumAbs], fabs(res));
        acc[kSumSum2] = dd_add_sq(acc[kSumSum2], both);
        acc[kSumObsPair] = dd_add_d(acc[kSumObsPair], ov);
        acc[kSumPredPair] = dd_add_d(acc[kSumPredPair], pv);
        acc[kSumObsPred] = dd_add_prod(acc[kSumObsPred], ov, pv);
      }
    }
  }

#pragma unroll
  for (int s = 0; s < kDetSums; ++s) {
    const dd v = dd_wave_sum(acc[s]);
    if (lane == 0) s_part[wave].sum[s] = v;
  }
#pragma unroll
  for (int s = 0; s < kDetCounts; ++s) {
    unsigned long long v = cnt[s];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    if (lane == 0) s_part[wave].count[s] = v;
  }
  __syncthreads();
  DetPartial *dst = partial + static_cast<size_t>(blockIdx.y) * gridDim.x + blockIdx.x;
  if (tid < kDetSums) {
    dd t = s_part[0].sum[tid];
    for (int w = 1; w < kDetThreads / 64; ++w) t = dd_add(t, s_part[w].sum[tid]);
    dst->sum[tid] = t;
  } else if (tid < kDetSums + kDetCounts) {
    const int s = tid - kDetSums;
    unsigned long long t = 0ull;
    for (int w = 0; w < kDetThreads / 64; ++w) t += s_part[w].count[s];
    dst->count[s] = t;
  }
}

// one wave per member: lane l adds partials l, l + 64, ... in that order, then the lanes are folded by dd_wave_sum
__global__ __launch_bounds__(64) void detcont_finish(const DetPartial *__restrict__ partial, int groups,
                                                     unsigned long long *__restrict__ counts, double *__restrict__ sums) {
  const DetPartial *src = partial + static_cast<size_t>(blockIdx.x) * groups;
  const int lane = threadIdx.x;
  for (int s = 0; s < kDetSums; ++s) {
    dd t = {0.0, 0.0};
    for (int g = lane; g < groups; g += 64) t = dd_add(t, src[g].sum[s]);
    t = dd_wave_sum(t);
    if (lane == 0) {
      sums[(static_cast<size_t>(blockIdx.x) * kDetSums + s) * 2] = t.hi;
      sums[(static_cast<size_t>(blockIdx.x) * kDetSums + s) * 2 + 1] = t.lo;
    }
  }
  for (int s = 0; s < kDetCounts; ++s) {
    unsigned long long t = 0ull;
    for (int g = lane; g < groups; g += 64) t += src[g].count[s];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) t += __shfl_xor(t, d);
    if (lane == 0) counts[static_cast<size_t>(blockIdx.x) * kDetCounts + s] = t;
  }
}

template <typename TF, typename TO>
int run_cat(const TF *fct, const TO *obs, int obs_shared, int K, size_t npix, const double *thr_f, const double *thr_o, int nthr,
            unsigned long long *out, hipStream_t s) {
  const dim3 grid(det_groups(npix), K);
  for (int t0 = 0; t0 < nthr; t0 += kDetThrBlock) {
    DetThresholds thr;
    thr.count = nthr - t0 < kDetThrBlock ? nthr - t0 : kDetThrBlock;
    for (int j = 0; j < kDetThrBlock; ++j) {
      thr.f[j] = j < thr.count ? thr_f[t0 + j] : 0.0;
      thr.o[j] = j < thr.count ? thr_o[t0 + j] : 0.0;
    }
    hipLaunchKernelGGL((detcat_count<TF, TO>), grid, dim3(kDetThreads), 0, s, fct, obs, obs_shared, npix, thr,
                       out + static_cast<size_t>(t0) * 4, static_cast<size_t>(nthr) * 4);
    PSH_HIP(hipGetLastError());
  }
  const size_t tables = static_cast<size_t>(K) * nthr;
  hipLaunchKernelGGL(detcat_finish, dim3(static_cast<unsigned>((tables + 255) / 256)), dim3(256), 0, s, out, tables,
                     static_cast<unsigned long long>(npix));
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

template <typename TF, typename TO>
int run_cont(const TF *fct, const TO *obs, int obs_shared, int K, size_t npix, int conditioning, double thr_f, double thr_o,
             DetPartial *partial, unsigned long long *counts, double *sums, hipStream_t s) {
  const int groups = det_groups(npix);
  hipLaunchKernelGGL((detcont_partial<TF, TO>), dim3(groups, K), dim3(kDetThreads), 0, s, fct, obs, obs_shared, npix,
                     conditioning, thr_f, thr_o, partial);
  PSH_HIP(hipGetLastError());
  hipLaunchKernelGGL(detcont_finish, dim3(K), dim3(64), 0, s, static_cast<const DetPartial *>(partial), groups, counts, sums);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

int check_fields(const char *what, const void *fct_dev, int fct_f64, const void *obs_dev, int obs_f64, int K, size_t npix) {
  if (!fct_dev || !obs_dev) return fail(PSH_EINVAL, "%s: NULL pointer", what);
  if (npix < 1) return fail(PSH_EINVAL, "%s: empty field", what);
  if (K < 1 || K > 65535) return fail(PSH_EINVAL, "%s: %d forecasts (1..65535)", what, K);
  if (reinterpret_cast<uintptr_t>(fct_dev) % (fct_f64 ? 8 : 4) || reinterpret_cast<uintptr_t>(obs_dev) % (obs_f64 ? 8 : 4))
    return fail(PSH_EINVAL, "%s: a field is not aligned to its element size", what);
  return PSH_OK;
}

}  // namespace
}  // namespace psh

using psh::fail;

extern "C" int psh_detcat_counts_dev(const void *fct_dev, int fct_f64, const void *obs_dev, int obs_f64, int obs_shared, int K,
                                     size_t npix, const double *thr_fct_host, const double *thr_obs_host, int n_thresholds,
                                     unsigned long long *out_dev) {
  using namespace psh;
  PSH_ENTER(c);
  if (!thr_fct_host || !thr_obs_host || !out_dev) return fail(PSH_EINVAL, "detcat: NULL pointer");
  if (int rc = check_fields("detcat", fct_dev, fct_f64, obs_dev, obs_f64, K, npix)) return rc;
  if (n_thresholds < 1 || n_thresholds > 4096) return fail(PSH_EINVAL, "detcat: %d thresholds (1..4096)", n_thresholds);
  PSH_HIP(hipMemsetAsync(out_dev, 0, static_cast<size_t>(K) * n_thresholds * 4 * sizeof(unsigned long long), c.stream));
  return with_real(fct_dev, fct_f64 != 0, [&](auto *fct) {
    return with_real(obs_dev, obs_f64 != 0, [&](auto *obs) {
      return run_cat(fct, obs, obs_shared, K, npix, thr_fct_host, thr_obs_host, n_thresholds, out_dev, c.stream);
    });
  });
}

extern "C" int psh_detcont_sums_dev(const void *fct_dev, int fct_f64, const void *obs_dev, int obs_f64, int obs_shared, int K,
                                    size_t npix, int conditioning, double thr_fct, double thr_obs,
                                    unsigned long long *counts_dev, double *sums_dev) {
  using namespace psh;
  PSH_ENTER(c);
  if (!counts_dev || !sums_dev) return fail(PSH_EINVAL, "detcont: NULL pointer");
  if (int rc = check_fields("detcont", fct_dev, fct_f64, obs_dev, obs_f64, K, npix)) return rc;
  if (conditioning < 0 || conditioning > 2) return fail(PSH_EINVAL, "detcont: conditioning %d (0 none, 1 single, 2 double)", conditioning);
  psh::Scratch blk;
  if (int rc = blk.alloc(static_cast<size_t>(K) * det_groups(npix) * sizeof(DetPartial))) return rc;
  DetPartial *part = blk.as<DetPartial>();
  return with_real(fct_dev, fct_f64 != 0, [&](auto *fct) {
    return with_real(obs_dev, obs_f64 != 0, [&](auto *obs) {
      return run_cont(fct, obs, obs_shared, K, npix, conditioning, thr_fct, thr_obs, part, counts_dev, sums_dev, c.stream);
    });
  });
}
