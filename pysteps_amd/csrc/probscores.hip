// Probabilistic verification on gfx950: what pysteps/verification/probscores.py CRPS_accum, reldiag_accum and
// ROC_curve_accum add to their objects, float32 or float64 fields each on its own.
//
//   crps_partial      Hersbach's decomposition of the CRPS of K members against an observation.  One thread owns a pixel
//                     for all members (member k of the 64 pixels of a wave is one coalesced load) and holds them in
//                     registers, padded with +inf to P = 8, 16, 32 or 64 values: the kernel is instantiated per P and
//                     every loop over the values is fully unrolled, so no register array is indexed dynamically (none
//                     goes to scratch).  The values are sorted by a bitonic network of min / max pairs, whose exchanges
//                     do not depend on the data: the 64 pixels of a wave never diverge, however many ties a rain field
//                     has, and there is no LDS traffic and no barrier.  The thread then walks the
//                     K + 1 bins with the reference's strict inequalities: between members i - 1 and i the bin adds
//                     alpha (i/K)^2 + beta ((K-i)/K)^2 with (alpha, beta) = (x_i - x_(i-1), 0) for x_o > x_i,
//                     (x_o - x_(i-1), x_i - x_o) for x_i > x_o > x_(i-1), (0, x_i - x_(i-1)) for x_o < x_(i-1) and
//                     nothing when x_o equals one of the two; the outer bins add (x_0 - x_o) for x_o < x_0 and
//                     (x_o - x_(K-1)) for x_(K-1) < x_o.  Differences are float64 operations on the widened values
//                     (exact for float32 input), the weights come from the caller's table, each product is rounded once
//                     and added to the thread's double-double sum (dd.h).  A pixel takes part when all K members and
//                     the observation are finite.  One partial per workgroup: the wave's sum by the fixed xor tree.
//   crps_finish       one wave per observation plane adds the partials in a fixed order.
//   probbins_partial  the bins of a reliability diagram and the contingency counts of a ROC curve in one read of a
//                     probability plane and its observation.  A thread owns a pixel: its bin is the number of edges
//                     below p (numpy.digitize(right=True); 0 and n_bins + 1 are no bin), counted against the edges the
//                     caller gave, and p is added to the thread's own double-double sum of that bin, which lives in a
//                     private LDS column (dynamic indexing without scratch, no conflicts, no barrier, pixel order).
//                     Counts need no order: per bin and per probability threshold one ballot over the wave, whose
//                     population counts (all pixels, and those with x_o >= x_min) lane b adds to the counters of bin b
//                     and threshold b.  At the end the 64 sums of a bin are folded by the fixed xor tree into lane b.
//                     No atomics, no dynamically indexed registers.
//   probbins_finish   one workgroup of 8 waves: wave w adds the partials w, w + 8, ... per lane, wave 0 the 8 results in
//                     wave order; misses and correct negatives follow from the numbers of valid pixels and of events.
// The pixel -> thread mapping and the grids depend on npix alone, and no floating-point atomics are used, so a result is
// the same bits in every run and wherever the plane lies in a stack.
#include "common.h"
#include "dd.h"

namespace psh {
namespace {

constexpr int kProbWave = 64;
constexpr int kCrpsMaxGroups = 4096;  // workgroups per plane - fixed: the summation order is part of the result
constexpr int kCrpsMaxMembers = 64;
constexpr int kBinsMaxGroups = 2048;
constexpr int kBinsLanes = 64;  // bins and probability thresholds a wave can own

struct CrpsPartial {
  dd sum;
  unsigned long long count;
};

template <typename T>
__device__ __forceinline__ T pos_inf();
template <>
__device__ __forceinline__ float pos_inf<float>() { return __builtin_inff(); }
template <>
__device__ __forceinline__ double pos_inf<double>() { return __builtin_inf(); }

__device__ __forceinline__ float lower(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ float upper(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double lower(double a, double b) { return fmin(a, b); }
__device__ __forceinline__ double upper(double a, double b) { return fmax(a, b); }

// grid (groups, planes), 64 threads.  P: K padded to 8, 16, 32 or 64; x[] is only ever indexed by unrolled loop
// counters, so it lives in registers.  weights: K + 1 pairs {(i/K)^2, ((K-i)/K)^2}.  partial[plane][group].
template <int P, typename TF, typename TO>
__global__ __launch_bounds__(kProbWave) void crps_partial(const TF *__restrict__ fct, size_t fct_stride, const TO *__restrict__ obs,
                                                          size_t npix, int K, const double *__restrict__ weights,
                                                          CrpsPartial *__restrict__ partial) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x;
  const TF *f = fct + static_cast<size_t>(blockIdx.y) * fct_stride;
  const TO *o = obs + static_cast<size_t>(blockIdx.y) * npix;
  dd acc = {0.0, 0.0};
  unsigned cnt = 0u;

  const size_t stride = static_cast<size_t>(gridDim.x) * kProbWave;
  for (size_t base = static_cast<size_t>(blockIdx.x) * kProbWave; base < npix; base += stride) {
    const size_t p = base + lane;
    const bool inside = p < npix;
    bool fin = inside;
    TF x[P];
#pragma unroll
    for (int k = 0; k < P; ++k) {
      if (k < K) {  // uniform
        x[k] = inside ? f[static_cast<size_t>(k) * npix + p] : static_cast<TF>(0);
        fin = fin && __builtin_isfinite(x[k]);
      } else {
        x[k] = pos_inf<TF>();
      }
    }
    const double xo = inside ? static_cast<double>(o[p]) : __builtin_nan("");
    fin = fin && __builtin_isfinite(xo);

    // bitonic network: pair c of a stage is (i, i + j), ascending where bit k2 of i is clear
#pragma unroll
    for (int k2 = 2; k2 <= P; k2 <<= 1) {
#pragma unroll
      for (int j = k2 >> 1; j > 0; j >>= 1) {
#pragma unroll
        for (int c = 0; c < (P >> 1); ++c) {
          const int i = ((c & ~(j - 1)) << 1) | (c & (j - 1));
          const TF a = x[i], b = x[i + j];
          const bool up = (i & k2) == 0;
          x[i] = up ? lower(a, b) : upper(a, b);
          x[i + j] = up ? upper(a, b) : lower(a, b);
        }
      }
    }

    if (fin) {
      cnt += 1u;
      double prev = static_cast<double>(x[0]);
      if (xo < prev) acc = dd_add_d(acc, (prev - xo) * weights[1]);
#pragma unroll
      for (int i = 1; i < P; ++i) {
        if (i < K) {  // uniform
          const double cur = static_cast<double>(x[i]);
          double alpha = 0.0, beta = 0.0;
          if (xo > cur) {
            alpha = cur - prev;
          } else if (xo > prev) {
            if (cur > xo) alpha = xo - prev, beta = cur - xo;
          } else if (xo < prev) {
            beta = cur - prev;
          }
          acc = dd_add_d(acc, alpha * weights[2 * i]);
          acc = dd_add_d(acc, beta * weights[2 * i + 1]);
          prev = cur;
        }
      }
      if (prev < xo) acc = dd_add_d(acc, (xo - prev) * weights[2 * K]);  // prev: member K - 1
    }
  }

  acc = dd_wave_sum(acc);
  unsigned long long total = cnt;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) total += __shfl_xor(total, d);
  if (lane == 0) {
    CrpsPartial *dst = partial + static_cast<size_t>(blockIdx.y) * gridDim.x + blockIdx.x;
    dst->sum = acc;
    dst->count = total;
  }
}

// one wave per plane: lane l adds partials l, l + 64, ... in that order, then the lanes are folded by dd_wave_sum
__global__ __launch_bounds__(kProbWave) void crps_finish(const CrpsPartial *__restrict__ partial, int groups,
                                                         unsigned long long *__restrict__ counts, double *__restrict__ sums) {
  const CrpsPartial *src = partial + static_cast<size_t>(blockIdx.x) * groups;
  const int lane = threadIdx.x;
  dd t = {0.0, 0.0};
  unsigned long long n = 0ull;
  for (int g = lane; g < groups; g += kProbWave) {
    t = dd_add(t, src[g].sum);
    n += src[g].count;
  }
  t = dd_wave_sum(t);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d);
  if (lane == 0) {
    counts[blockIdx.x] = n;
    sums[static_cast<size_t>(blockIdx.x) * 2] = t.hi;
    sums[static_cast<size_t>(blockIdx.x) * 2 + 1] = t.lo;
  }
}

struct BinsPartial {
  double hi[kBinsLanes], lo[kBinsLanes];
  unsigned cnt[kBinsLanes], ycnt[kBinsLanes], hits[kBinsLanes], fa[kBinsLanes];
  unsigned long long valid, events;
};

// grid (groups), 64 threads, n_bins * 1024 bytes of LDS: the threads' private double-double sums, (hi, lo) of bin b and
// thread t at (2 b) * 64 + t and (2 b + 1) * 64 + t.  tables: kBinsLanes + 1 slots of bin edges, then the probability
// thresholds.
template <typename TP, typename TO>
__global__ __launch_bounds__(kProbWave) void probbins_partial(const TP *__restrict__ prob, const TO *__restrict__ obs, size_t npix,
                                                              double x_min, const double *__restrict__ tables, int n_bins, int n_thr,
                                                              BinsPartial *__restrict__ partial) {
  extern __shared__ double bin_columns[];
  const int lane = threadIdx.x;
  double *col = bin_columns + lane;
  const double *thrs = tables + kBinsLanes + 1;
  for (int b = 0; b < 2 * n_bins; ++b) col[b * kProbWave] = 0.0;
  unsigned cnt = 0u, ycnt = 0u, hits = 0u, fa = 0u;
  unsigned long long valid_total = 0ull, event_total = 0ull;

  const size_t stride = static_cast<size_t>(gridDim.x) * kProbWave;
  for (size_t base = static_cast<size_t>(blockIdx.x) * kProbWave; base < npix; base += stride) {
    const size_t idx = base + lane;
    const bool inside = idx < npix;
    const double p = inside ? static_cast<double>(prob[idx]) : __builtin_nan("");
    const double o = inside ? static_cast<double>(obs[idx]) : __builtin_nan("");
    const bool valid = __builtin_isfinite(p) && __builtin_isfinite(o);
    const unsigned long long events = __ballot(valid && o >= x_min);
    valid_total += __popcll(__ballot(valid));
    event_total += __popcll(events);
    if (n_bins) {  // uniform
      int below = 0;  // the number of edges below p: numpy.digitize(p, edges, right=True)
      for (int e = 0; e <= n_bins; ++e) below += tables[e] < p ? 1 : 0;
      const int bin = (valid && below >= 1 && below <= n_bins) ? below - 1 : -1;
      if (bin >= 0) {
        double *slot = col + 2 * bin * kProbWave;
        const dd sum = dd_add_d(dd{slot[0], slot[kProbWave]}, p);
        slot[0] = sum.hi;
        slot[kProbWave] = sum.lo;
      }
      for (int b = 0; b < n_bins; ++b) {
        const unsigned long long members = __ballot(bin == b);
        cnt += lane == b ? __popcll(members) : 0;
        ycnt += lane == b ? __popcll(members & events) : 0;
      }
    }
    for (int i = 0; i < n_thr; ++i) {
      const unsigned long long yes = __ballot(valid && p >= thrs[i]);
      hits += lane == i ? __popcll(yes & events) : 0;
      fa += lane == i ? __popcll(yes & ~events) : 0;
    }
  }

  dd sum = {0.0, 0.0};
  for (int b = 0; b < n_bins; ++b) {  // the 64 threads' sums of bin b, folded by the fixed xor tree, go to lane b
    const dd v = dd_wave_sum(dd{col[2 * b * kProbWave], col[(2 * b + 1) * kProbWave]});
    if (lane == b) sum = v;
  }
  BinsPartial *dst = partial + blockIdx.x;
  dst->hi[lane] = sum.hi;
  dst->lo[lane] = sum.lo;
  dst->cnt[lane] = cnt;
  dst->ycnt[lane] = ycnt;
  dst->hits[lane] = hits;
  dst->fa[lane] = fa;
  if (lane == 0) {
    dst->valid = valid_total;
    dst->events = event_total;
  }
}

// one workgroup of kFinishWaves waves: wave w adds the partials w, w + kFinishWaves, ... of every lane in that order, wave 0
// then adds the waves' results in wave order.  bins (n_bins, 2) {count, count of x_o >= x_min}, sums (n_bins, 2) {hi, lo},
// roc (n_thr, 4) {hits, misses, false alarms, correct negatives}
constexpr int kFinishWaves = 8;
__global__ __launch_bounds__(kFinishWaves *kProbWave) void probbins_finish(const BinsPartial *__restrict__ partial, int groups, int n_bins,
                                                                          int n_thr, unsigned long long *__restrict__ bins,
                                                                          double *__restrict__ sums, unsigned long long *__restrict__ roc) {
  __shared__ dd s_sum[kFinishWaves][kBinsLanes];
  __shared__ unsigned long long s_cnt[kFinishWaves][6][kBinsLanes];
  const int lane = threadIdx.x & (kProbWave - 1), wave = threadIdx.x / kProbWave;
  dd t = {0.0, 0.0};
  unsigned long long c[6] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};  // count, events in bin, hits, false alarms, valid, events
  for (int g = wave; g < groups; g += kFinishWaves) {
    const BinsPartial &s = partial[g];
    t = dd_add(t, dd{s.hi[lane], s.lo[lane]});
    c[0] += s.cnt[lane];
    c[1] += s.ycnt[lane];
    c[2] += s.hits[lane];
    c[3] += s.fa[lane];
    c[4] += s.valid;
    c[5] += s.events;
  }
  s_sum[wave][lane] = t;
#pragma unroll
  for (int k = 0; k < 6; ++k) s_cnt[wave][k][lane] = c[k];
  __syncthreads();
  if (wave != 0) return;
  for (int w = 1; w < kFinishWaves; ++w) {
    t = dd_add(t, s_sum[w][lane]);
#pragma unroll
    for (int k = 0; k < 6; ++k) c[k] += s_cnt[w][k][lane];
  }
  if (lane < n_bins) {
    bins[lane * 2] = c[0];
    bins[lane * 2 + 1] = c[1];
    sums[lane * 2] = t.hi;
    sums[lane * 2 + 1] = t.lo;
  }
  if (lane < n_thr) {
    roc[lane * 4] = c[2];
    roc[lane * 4 + 1] = c[5] - c[2];
    roc[lane * 4 + 2] = c[3];
    roc[lane * 4 + 3] = (c[4] - c[5]) - c[3];
  }
}

int groups_of(size_t npix, int most) {
  const size_t groups = (npix + kProbWave - 1) / kProbWave;
  return static_cast<int>(groups < static_cast<size_t>(most) ? groups : most);
}

template <int P, typename TF, typename TO>
void launch_crps(const TF *fct, size_t fct_stride, const TO *obs, int planes, int K, size_t npix, const double *weights_dev,
                 CrpsPartial *partial, int groups, hipStream_t s) {
  hipLaunchKernelGGL((crps_partial<P, TF, TO>), dim3(groups, planes), dim3(kProbWave), 0, s, fct, fct_stride, obs, npix, K,
                     weights_dev, partial);
}

template <typename TF, typename TO>
int run_crps(const TF *fct, size_t fct_stride, const TO *obs, int planes, int K, size_t npix, const double *weights_dev,
             CrpsPartial *partial, unsigned long long *counts, double *sums, hipStream_t s) {
  const int groups = groups_of(npix, kCrpsMaxGroups);
  if (K <= 8)
    launch_crps<8>(fct, fct_stride, obs, planes, K, npix, weights_dev, partial, groups, s);
  else if (K <= 16)
    launch_crps<16>(fct, fct_stride, obs, planes, K, npix, weights_dev, partial, groups, s);
  else if (K <= 32)
    launch_crps<32>(fct, fct_stride, obs, planes, K, npix, weights_dev, partial, groups, s);
  else
    launch_crps<kCrpsMaxMembers>(fct, fct_stride, obs, planes, K, npix, weights_dev, partial, groups, s);
  PSH_HIP(hipGetLastError());
  hipLaunchKernelGGL(crps_finish, dim3(planes), dim3(kProbWave), 0, s, static_cast<const CrpsPartial *>(partial), groups, counts,
                     sums);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

template <typename TP, typename TO>
int run_bins(const TP *prob, const TO *obs, size_t npix, double x_min, const double *tables_dev, int n_bins, int n_thr,
             BinsPartial *partial, unsigned long long *bins, double *sums, unsigned long long *roc, hipStream_t s) {
  const int groups = groups_of(npix, kBinsMaxGroups);
  hipLaunchKernelGGL((probbins_partial<TP, TO>), dim3(groups), dim3(kProbWave), static_cast<size_t>(n_bins) * 2 * kProbWave * sizeof(double),
                     s, prob, obs, npix, x_min, tables_dev, n_bins, n_thr, partial);
  PSH_HIP(hipGetLastError());
  hipLaunchKernelGGL(probbins_finish, dim3(1), dim3(kFinishWaves * kProbWave), 0, s, static_cast<const BinsPartial *>(partial), groups, n_bins,
                     n_thr, bins, sums, roc);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

// per-call constants through the pinned slot ring (floats: two per double); `fill` writes `count` doubles
template <class Fill>
int upload_doubles(size_t count, const double **dev, Fill fill) {
  static_assert(kConstSlotFloats >= 2 * 3 * kBinsLanes && kConstSlotFloats >= 4 * (kCrpsMaxMembers + 1), "slot too small");
  float *h = nullptr;
  const float *d = nullptr;
  if (int rc = const_slot(&h, &d)) return rc;
  fill(reinterpret_cast<double *>(h));
  PSH_HIP(hipMemcpyAsync(const_cast<float *>(d), h, count * sizeof(double), hipMemcpyHostToDevice, ctx().stream));
  *dev = reinterpret_cast<const double *>(d);
  return PSH_OK;
}

bool misaligned(const void *p, int f64) { return reinterpret_cast<uintptr_t>(p) % (f64 ? 8 : 4) != 0; }

}  // namespace
}  // namespace psh

using psh::fail;

extern "C" int psh_crps_sums_dev(const void *fct_dev, int fct_f64, int fct_shared, const void *obs_dev, int obs_f64, int n_planes,
                                 int K, size_t npix, const double *weights_host, unsigned long long *counts_dev,
                                 double *sums_dev) {
  using namespace psh;
  PSH_ENTER(c);
  if (!fct_dev || !obs_dev || !weights_host || !counts_dev || !sums_dev) return fail(PSH_EINVAL, "crps: NULL pointer");
  if (npix < 1) return fail(PSH_EINVAL, "crps: empty field");
  if (K < 1 || K > kCrpsMaxMembers) return fail(PSH_EINVAL, "crps: %d members (1..%d)", K, kCrpsMaxMembers);
  if (n_planes < 1 || n_planes > 65535) return fail(PSH_EINVAL, "crps: %d observation planes (1..65535)", n_planes);
  if (misaligned(fct_dev, fct_f64) || misaligned(obs_dev, obs_f64))
    return fail(PSH_EINVAL, "crps: a field is not aligned to its element size");
  const double *weights = nullptr;
  if (int rc = upload_doubles(static_cast<size_t>(K + 1) * 2, &weights, [&](double *h) {
        for (int i = 0; i < 2 * (K + 1); ++i) h[i] = weights_host[i];
      }))
    return rc;
  psh::Scratch blk;
  if (int rc = blk.alloc(static_cast<size_t>(n_planes) * groups_of(npix, kCrpsMaxGroups) * sizeof(CrpsPartial))) return rc;
  CrpsPartial *part = blk.as<CrpsPartial>();
  const size_t stride = fct_shared ? 0 : static_cast<size_t>(K) * npix;
  return with_real(fct_dev, fct_f64 != 0, [&](auto *fct) {
    return with_real(obs_dev, obs_f64 != 0, [&](auto *obs) {
      return run_crps(fct, stride, obs, n_planes, K, npix, weights, part, counts_dev, sums_dev, c.stream);
    });
  });
}

extern "C" int psh_probbins_dev(const void *prob_dev, int prob_f64, const void *obs_dev, int obs_f64, size_t npix, double x_min,
                                const double *edges_host, int n_edges, const double *prob_thrs_host, int n_prob_thrs,
                                unsigned long long *bins_dev, double *sums_dev, unsigned long long *roc_dev) {
  using namespace psh;
  PSH_ENTER(c);
  if (!prob_dev || !obs_dev) return fail(PSH_EINVAL, "probbins: NULL pointer");
  if (npix < 1) return fail(PSH_EINVAL, "probbins: empty field");
  if (n_edges < 0 || n_edges == 1 || n_edges > kBinsLanes + 1)
    return fail(PSH_EINVAL, "probbins: %d bin edges (0, or 2..%d)", n_edges, kBinsLanes + 1);
  if (n_prob_thrs < 0 || n_prob_thrs > kBinsLanes)
    return fail(PSH_EINVAL, "probbins: %d probability thresholds (0..%d)", n_prob_thrs, kBinsLanes);
  const int n_bins = n_edges ? n_edges - 1 : 0;
  if (!n_bins && !n_prob_thrs) return fail(PSH_EINVAL, "probbins: neither bins nor probability thresholds");
  if ((n_bins && (!edges_host || !bins_dev || !sums_dev)) || (n_prob_thrs && (!prob_thrs_host || !roc_dev)))
    return fail(PSH_EINVAL, "probbins: NULL pointer");
  if (misaligned(prob_dev, prob_f64) || misaligned(obs_dev, obs_f64))
    return fail(PSH_EINVAL, "probbins: a field is not aligned to its element size");
  const double *tables = nullptr;
  if (int rc = upload_doubles(static_cast<size_t>(2) * kBinsLanes + 1, &tables, [&](double *h) {
        for (int e = 0; e <= kBinsLanes; ++e) h[e] = e < n_edges ? edges_host[e] : NAN;
        for (int i = 0; i < kBinsLanes; ++i) h[kBinsLanes + 1 + i] = i < n_prob_thrs ? prob_thrs_host[i] : NAN;
      }))
    return rc;
  psh::Scratch blk;
  if (int rc = blk.alloc(static_cast<size_t>(groups_of(npix, kBinsMaxGroups)) * sizeof(BinsPartial))) return rc;
  BinsPartial *part = blk.as<BinsPartial>();
  return with_real(prob_dev, prob_f64 != 0, [&](auto *prob) {
    return with_real(obs_dev, obs_f64 != 0, [&](auto *obs) {
      return run_bins(prob, obs, npix, x_min, tables, n_bins, n_prob_thrs, part, bins_dev, sums_dev, roc_dev, c.stream);
    });
  });
}
