// Ensemble spread on gfx950: the deterministic scores of pysteps/verification/ensscores.py ensemble_spread between all
// K (K - 1) / 2 pairs of the members of a stack (K, npix), float32 or float64, in one pass.  Pairs are numbered in the
// reference's loop order: (0, 1), (0, 2), ..., (0, K - 1), (1, 2), ...; member i is the prediction, member j the
// observation.
//
//   detcat_pairs    one wave per workgroup walks 64-pixel steps; lane l loads pixel l of every member (one coalesced
//                   load per member).  Per threshold the event bits x > thr of a member's 64 pixels are one ballot
//                   (NaN compares false, a pixel beyond npix is NaN), which lane m keeps for member m and puts into
//                   the wave's LDS row.  Lane l then serves the pairs l, l + 64, ...: hits += popcount(b_i & b_j),
//                   with the (i, j) of its Q pairs in registers from the start and 32-bit counters in registers; lane
//                   m also counts the events of member m.  The kernel is instantiated per Q = 2, 8, 18, 32 pairs per
//                   lane (K <= 16, 32, 48, 64) and thresholds per pass (8, or 4 at Q = 32), so no register array is
//                   indexed dynamically.  False alarms, misses and correct negatives of a pair follow on the host from
//                   hits, the two event counts and npix.  One row of counters per wave goes to memory.
//   detcat_pairs_finish  adds the waves' rows as 64-bit integers.  Integer adds commute: no order to keep, no atomics.
//   detcont_pairs   a workgroup serves a TT x TT tile of members for the chunks detcont_partial (detscores.hip) gives
//                   it: chunk c of four pixels to thread c % (groups * 256), det_groups(npix) workgroups.  A thread
//                   reads 2 TT members for TT^2 pairs and carries the NS sums that sum_mask selects as double-double
//                   pairs, each with detcont_partial's term and in its order: per thread sequential, dd_wave_sum, the
//                   waves in wave order.  TT = 4 for one or two sums, TT = 2 for more; the slot is a compile-time
//                   index, and which sum it carries picks the term's operands by scalar conditions on the uniform
//                   mask.  A diagonal tile does only i < j, and members beyond K none.
//   detcont_pairs_finish  one wave per pair adds the workgroups' partials in detcont_finish's lane order.
// A pair's sums are therefore the bits psh_detcont_sums_dev returns for (plane i, plane j), in every run and wherever
// the stack lies.  No floating-point atomics.
#include "common.h"
#include "dd.h"
#include "detsums.h"

namespace psh {
namespace {

constexpr int kPairMaxMembers = 64;
constexpr int kPairMaxWaves = 2048;  // workgroups of detcat_pairs: 8 waves on each of 256 compute units
constexpr int kPairMaxThrBlock = 8;

struct PairThresholds {
  double v[kPairMaxThrBlock];
  int count;
};

// grid (waves), 64 threads.  partial[wave][TB][Q * 64 + 64]: hits of pair p at column p, events of member m at column
// Q * 64 + m.
template <int Q, int TB, typename T>
__global__ __launch_bounds__(64) void detcat_pairs(const T *__restrict__ stack, int K, size_t npix, int npairs, PairThresholds thr,
                                                   unsigned *__restrict__ partial) {
  __shared__ unsigned long long row[TB][64];
  const int lane = threadIdx.x;
  // the pairs of this lane: p = lane + 64 q is the (p - start_i)-th pair of member i, whose pairs start at start_i
  int pi[Q], pj[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int p = lane + 64 * q;
    int i = 0, start = 0;
    if (p < npairs) {
      while (start + (K - 1 - i) <= p) start += K - 1 - i, ++i;
      pi[q] = i, pj[q] = i + 1 + (p - start);
    } else {
      pi[q] = pj[q] = 0;  // counted, never stored
    }
  }
  unsigned hits[TB][Q], events[TB];
#pragma unroll
  for (int t = 0; t < TB; ++t) {
    events[t] = 0u;
#pragma unroll
    for (int q = 0; q < Q; ++q) hits[t][q] = 0u;
  }

  const size_t nsteps = (npix + 63) / 64;
  for (size_t s = blockIdx.x; s < nsteps; s += gridDim.x) {
    const size_t px = s * 64 + lane;
    const bool inside = px < npix;
    unsigned long long mine[TB];
#pragma unroll
    for (int t = 0; t < TB; ++t) mine[t] = 0ull;
    for (int m0 = 0; m0 < K; m0 += 8) {
      double x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        x[u] = (inside && m0 + u < K) ? static_cast<double>(stack[static_cast<size_t>(m0 + u) * npix + px]) : quiet_nan();
#pragma unroll
      for (int u = 0; u < 8; ++u) {
#pragma unroll
        for (int t = 0; t < TB; ++t) {
          if (t < thr.count) {  // uniform
            const unsigned long long b = __ballot(x[u] > thr.v[t]);  // NaN: false
            if (lane == m0 + u) mine[t] = b;
          }
        }
      }
    }
    __syncthreads();  // the row of the step before has been read
#pragma unroll
    for (int t = 0; t < TB; ++t) {
      row[t][lane] = mine[t];
      events[t] += static_cast<unsigned>(__popcll(mine[t]));
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < TB; ++t) {
      if (t < thr.count) {
#pragma unroll
        for (int q = 0; q < Q; ++q) hits[t][q] += static_cast<unsigned>(__popcll(row[t][pi[q]] & row[t][pj[q]]));
      }
    }
  }

  unsigned *dst = partial + static_cast<size_t>(blockIdx.x) * TB * (Q * 64 + 64);
#pragma unroll
  for (int t = 0; t < TB; ++t) {
#pragma unroll
    for (int q = 0; q < Q; ++q) dst[t * (Q * 64 + 64) + q * 64 + lane] = hits[t][q];
    dst[t * (Q * 64 + 64) + Q * 64 + lane] = events[t];
  }
}

// grid (columns / 256, thresholds of the pass); hits and events point at the first threshold of the pass
__global__ __launch_bounds__(256) void detcat_pairs_finish(const unsigned *__restrict__ partial, int waves, int block_thr, int columns,
                                                           int pair_columns, int npairs, int K,
                                                           unsigned long long *__restrict__ hits,
                                                           unsigned long long *__restrict__ events) {
  const int col = blockIdx.x * blockDim.x + threadIdx.x, t = blockIdx.y;
  if (col >= columns) return;
  const bool is_pair = col < npairs, is_member = col >= pair_columns && col - pair_columns < K;
  if (!is_pair && !is_member) return;
  unsigned long long sum = 0ull;
  for (int w = 0; w < waves; ++w) sum += partial[(static_cast<size_t>(w) * block_thr + t) * columns + col];
  if (is_pair)
    hits[static_cast<size_t>(t) * npairs + col] = sum;
  else
    events[static_cast<size_t>(t) * K + (col - pair_columns)] = sum;
}

template <int TT, int NS>
struct PairPartial {
  dd sum[TT * TT][NS];
  unsigned long long count[TT * TT];
};

__host__ __device__ inline int tiles_before(int ti, int nt) { return ti * nt - ti * (ti - 1) / 2; }  // of the upper triangle

// grid (groups, tiles of the upper triangle); partial[tile][group]
template <int TT, int NS, typename T>
__global__ __launch_bounds__(kDetThreads) void detcont_pairs(const T *__restrict__ stack, int K, size_t npix, int sum_mask,
                                                             PairPartial<TT, NS> *__restrict__ partial) {
#pragma clang fp contract(off)
  constexpr int P = TT * TT;
  static_assert(P * 4 <= 64, "the finite-pair bits of a chunk fill one 64-bit word");
  __shared__ PairPartial<TT, NS> s_part[kDetThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nt = (K + TT - 1) / TT;
  int ti = 0, rest = blockIdx.y;
  while (rest >= nt - ti) rest -= nt - ti, ++ti;
  const int tj = ti + rest;

  int kind[NS];  // the sum slot k carries, -1: none
  {
    int m = sum_mask;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      kind[k] = m ? __builtin_ctz(m) : -1;
      m &= m - 1;
    }
  }
  const T *pred[TT], *obs[TT];
  bool vec_p[TT], vec_o[TT], served[P];
#pragma unroll
  for (int a = 0; a < TT; ++a) {
    const int i = ti * TT + a, j = tj * TT + a;
    pred[a] = stack + static_cast<size_t>(i < K ? i : K - 1) * npix;
    obs[a] = stack + static_cast<size_t>(j < K ? j : K - 1) * npix;
    vec_p[a] = aligned16(pred[a]), vec_o[a] = aligned16(obs[a]);
  }
#pragma unroll
  for (int a = 0; a < TT; ++a)
#pragma unroll
    for (int b = 0; b < TT; ++b) served[a * TT + b] = ti * TT + a < tj * TT + b && tj * TT + b < K;  // uniform

  dd acc[P][NS];
  unsigned cnt[P];
#pragma unroll
  for (int pr = 0; pr < P; ++pr) {
    cnt[pr] = 0u;
#pragma unroll
    for (int k = 0; k < NS; ++k) acc[pr][k] = {0.0, 0.0};
  }

  const size_t nchunk = (npix + 3) / 4, stride = static_cast<size_t>(gridDim.x) * kDetThreads;
  for (size_t c = static_cast<size_t>(blockIdx.x) * kDetThreads + tid; c < nchunk; c += stride) {
    double p[TT][4], q[TT][4];
#pragma unroll
    for (int a = 0; a < TT; ++a) {
      load4(pred[a], c * 4, npix, vec_p[a], p[a]);
      load4(obs[a], c * 4, npix, vec_o[a], q[a]);
    }
    unsigned long long ok = 0ull;  // bit pr * 4 + e: the pair's residual at element e is finite
#pragma unroll
    for (int pr = 0; pr < P; ++pr) {
      if (served[pr]) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const double pv = p[pr / TT][e], ov = q[pr % TT][e];
          const bool fin = __builtin_isfinite(ov) && __builtin_isfinite(pv) && __builtin_isfinite(pv - ov);
          ok |= static_cast<unsigned long long>(fin) << (pr * 4 + e);
          cnt[pr] += fin ? 1u : 0u;
        }
      }
    }
    // every finite pair of the chunk, element by element as detcont_partial adds them.  A sum is a + x (dd_add_d) or
    // a + x * y with the product exact (dd_add_prod; dd_add_sq(a, v) is dd_add_prod(a, v, v) operation by operation);
    // which one and of what is uniform, so the operands are picked by scalar conditions and the bits are the term's own
#define PSH_PAIR_SUM(...)                                                               \
  _Pragma("unroll") for (int pr = 0; pr < P; ++pr) {                                    \
    if (served[pr]) {                                                                   \
      _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                   \
        if ((ok >> (pr * 4 + e)) & 1ull) {                                              \
          const double pv = p[pr / TT][e], ov = q[pr % TT][e];                          \
          __VA_ARGS__                                                                   \
        }                                                                               \
      }                                                                                 \
    }                                                                                   \
  }
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int kd = kind[k];
      if (kd == kSumRes2 || kd == kSumSum2 || kd == kSumObsPred) {
        PSH_PAIR_SUM(const double x = kd == kSumRes2 ? pv - ov : kd == kSumSum2 ? pv + ov : ov;
                     acc[pr][k] = dd_add_prod(acc[pr][k], x, kd == kSumObsPred ? pv : x);)
      } else if (kd >= 0) {
        PSH_PAIR_SUM(const double res = pv - ov;
                     acc[pr][k] = dd_add_d(acc[pr][k], kd == kSumRes ? res : kd == kSumAbs ? fabs(res) : kd == kSumObsPair ? ov : pv);)
      }
    }
#undef PSH_PAIR_SUM
  }

#pragma unroll
  for (int pr = 0; pr < P; ++pr) {
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const dd v = dd_wave_sum(acc[pr][k]);
      if (lane == 0) s_part[wave].sum[pr][k] = v;
    }
    unsigned long long v = cnt[pr];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    if (lane == 0) s_part[wave].count[pr] = v;
  }
  __syncthreads();
  PairPartial<TT, NS> *dst = partial + static_cast<size_t>(blockIdx.y) * gridDim.x + blockIdx.x;
  if (tid < P * NS) {
    const int pr = tid / NS, k = tid % NS;
    dd t = s_part[0].sum[pr][k];
    for (int w = 1; w < kDetThreads / 64; ++w) t = dd_add(t, s_part[w].sum[pr][k]);
    dst->sum[pr][k] = t;
  } else if (tid < P * NS + P) {
    const int pr = tid - P * NS;
    unsigned long long t = 0ull;
    for (int w = 0; w < kDetThreads / 64; ++w) t += s_part[w].count[pr];
    dst->count[pr] = t;
  }
}

// one wave per pair: lane l adds partials l, l + 64, ... in that order, then the lanes are folded by dd_wave_sum - the
// order of detcont_finish.  Sums that sum_mask does not select are zeros.
template <int TT, int NS>
__global__ __launch_bounds__(64) void detcont_pairs_finish(const PairPartial<TT, NS> *__restrict__ partial, int groups, int K, int sum_mask,
                                                           unsigned long long *__restrict__ counts, double *__restrict__ sums) {
  const int lane = threadIdx.x, nt = (K + TT - 1) / TT;
  int i = 0, rest = blockIdx.x;
  while (rest >= K - 1 - i) rest -= K - 1 - i, ++i;
  const int j = i + 1 + rest, pr = (i % TT) * TT + j % TT;
  const PairPartial<TT, NS> *src = partial + static_cast<size_t>(tiles_before(i / TT, nt) + (j / TT - i / TT)) * groups;
  for (int s = 0; s < kPairSums; ++s) {
    const int k = __builtin_popcount(sum_mask & ((1 << s) - 1));
    dd t = {0.0, 0.0};
    if ((sum_mask >> s) & 1) {
      for (int g = lane; g < groups; g += 64) t = dd_add(t, src[g].sum[pr][k]);
      t = dd_wave_sum(t);
    }
    if (lane == 0) {
      sums[(static_cast<size_t>(blockIdx.x) * kPairSums + s) * 2] = t.hi;
      sums[(static_cast<size_t>(blockIdx.x) * kPairSums + s) * 2 + 1] = t.lo;
    }
  }
  unsigned long long t = 0ull;
  for (int g = lane; g < groups; g += 64) t += src[g].count[pr];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) t += __shfl_xor(t, d);
  if (lane == 0) counts[blockIdx.x] = t;
}

template <int Q, int TB, typename T>
int run_cat_pairs(const T *stack, int K, size_t npix, const double *thr, int nthr, unsigned *partial, unsigned long long *hits,
                  unsigned long long *events, hipStream_t s) {
  const int npairs = K * (K - 1) / 2, columns = Q * 64 + 64;
  const size_t nsteps = (npix + 63) / 64;
  const int waves = static_cast<int>(nsteps < static_cast<size_t>(kPairMaxWaves) ? nsteps : kPairMaxWaves);
  for (int t0 = 0; t0 < nthr; t0 += TB) {
    PairThresholds block;
    block.count = nthr - t0 < TB ? nthr - t0 : TB;
    for (int t = 0; t < kPairMaxThrBlock; ++t) block.v[t] = t < block.count ? thr[t0 + t] : 0.0;
    hipLaunchKernelGGL((detcat_pairs<Q, TB, T>), dim3(waves), dim3(64), 0, s, stack, K, npix, npairs, block, partial);
    PSH_HIP(hipGetLastError());
    hipLaunchKernelGGL(detcat_pairs_finish, dim3((columns + 255) / 256, block.count), dim3(256), 0, s,
                       static_cast<const unsigned *>(partial), waves, TB, columns, Q * 64, npairs, K,
                       hits + static_cast<size_t>(t0) * npairs, events + static_cast<size_t>(t0) * K);
    PSH_HIP(hipGetLastError());
  }
  return PSH_OK;
}

// pairs per lane and thresholds per pass by ensemble size: 32 x 4 and 18 x 8 counters stay in registers
size_t cat_pairs_partial_bytes(int K, size_t npix) {
  const int Q = K <= 16 ? 2 : K <= 32 ? 8 : K <= 48 ? 18 : 32, TB = K <= 48 ? 8 : 4;
  const size_t nsteps = (npix + 63) / 64;
  const size_t waves = nsteps < static_cast<size_t>(kPairMaxWaves) ? nsteps : kPairMaxWaves;
  return waves * TB * (Q * 64 + 64) * sizeof(unsigned);
}

template <int TT, int NS, typename T>
int run_cont_pairs(const T *stack, int K, size_t npix, int sum_mask, void *partial, unsigned long long *counts, double *sums,
                   hipStream_t s) {
  const int groups = det_groups(npix), nt = (K + TT - 1) / TT;
  auto *part = static_cast<PairPartial<TT, NS> *>(partial);
  hipLaunchKernelGGL((detcont_pairs<TT, NS, T>), dim3(groups, tiles_before(nt, nt)), dim3(kDetThreads), 0, s, stack, K, npix, sum_mask,
                     part);
  PSH_HIP(hipGetLastError());
  hipLaunchKernelGGL((detcont_pairs_finish<TT, NS>), dim3(K * (K - 1) / 2), dim3(64), 0, s, static_cast<const PairPartial<TT, NS> *>(part),
                     groups, K, sum_mask, counts, sums);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

// tile side and slots by the number of selected sums: 16 pairs x 2 sums and 4 pairs x 7 sums fit the registers
template <int TT, int NS>
size_t cont_pairs_partial_bytes(int K, size_t npix) {
  const int nt = (K + TT - 1) / TT;
  return static_cast<size_t>(tiles_before(nt, nt)) * det_groups(npix) * sizeof(PairPartial<TT, NS>);
}

int check_stack(const char *what, const void *stack_dev, int f64, int K, size_t npix) {
  if (!stack_dev) return fail(PSH_EINVAL, "%s: NULL pointer", what);
  if (npix < 1 || npix >= (static_cast<size_t>(1) << 40)) return fail(PSH_EINVAL, "%s: %zu pixels (1..2^40 - 1)", what, npix);
  if (K < 2 || K > kPairMaxMembers) return fail(PSH_EINVAL, "%s: %d members (2..%d)", what, K, kPairMaxMembers);
  if (reinterpret_cast<uintptr_t>(stack_dev) % (f64 ? 8 : 4)) return fail(PSH_EINVAL, "%s: the stack is not aligned to its element size", what);
  return PSH_OK;
}

}  // namespace
}  // namespace psh

using psh::fail;

extern "C" int psh_detcat_pairs_dev(const void *stack_dev, int f64, int K, size_t npix, const double *thr_host, int n_thresholds,
                                    unsigned long long *hits_dev, unsigned long long *events_dev) {
  using namespace psh;
  PSH_ENTER(c);
  if (!thr_host || !hits_dev || !events_dev) return fail(PSH_EINVAL, "detcat pairs: NULL pointer");
  if (int rc = check_stack("detcat pairs", stack_dev, f64, K, npix)) return rc;
  if (n_thresholds < 1 || n_thresholds > 4096) return fail(PSH_EINVAL, "detcat pairs: %d thresholds (1..4096)", n_thresholds);
  psh::Scratch blk;
  if (int rc = blk.alloc(cat_pairs_partial_bytes(K, npix))) return rc;
  unsigned *part = blk.as<unsigned>();
  return with_real(stack_dev, f64 != 0, [&](auto *stack) {
    if (K <= 16) return run_cat_pairs<2, 8>(stack, K, npix, thr_host, n_thresholds, part, hits_dev, events_dev, c.stream);
    if (K <= 32) return run_cat_pairs<8, 8>(stack, K, npix, thr_host, n_thresholds, part, hits_dev, events_dev, c.stream);
    if (K <= 48) return run_cat_pairs<18, 8>(stack, K, npix, thr_host, n_thresholds, part, hits_dev, events_dev, c.stream);
    return run_cat_pairs<32, 4>(stack, K, npix, thr_host, n_thresholds, part, hits_dev, events_dev, c.stream);
  });
}

extern "C" int psh_detcont_pairs_dev(const void *stack_dev, int f64, int K, size_t npix, int sum_mask,
                                     unsigned long long *counts_dev, double *sums_dev) {
  using namespace psh;
  PSH_ENTER(c);
  if (!counts_dev || !sums_dev) return fail(PSH_EINVAL, "detcont pairs: NULL pointer");
  if (int rc = check_stack("detcont pairs", stack_dev, f64, K, npix)) return rc;
  if (sum_mask < 1 || sum_mask >= (1 << kPairSums)) return fail(PSH_EINVAL, "detcont pairs: sum mask %d (1..%d)", sum_mask, (1 << kPairSums) - 1);
  const int selected = __builtin_popcount(sum_mask);
  psh::Scratch blk;
  if (int rc = blk.alloc(selected == 1   ? cont_pairs_partial_bytes<4, 1>(K, npix)
                         : selected == 2 ? cont_pairs_partial_bytes<4, 2>(K, npix)
                         : selected == 3 ? cont_pairs_partial_bytes<2, 3>(K, npix)
                                         : cont_pairs_partial_bytes<2, 7>(K, npix)))
    return rc;
  void *part = blk.as<void>();
  return with_real(stack_dev, f64 != 0, [&](auto *stack) {
    if (selected == 1) return run_cont_pairs<4, 1>(stack, K, npix, sum_mask, part, counts_dev, sums_dev, c.stream);
    if (selected == 2) return run_cont_pairs<4, 2>(stack, K, npix, sum_mask, part, counts_dev, sums_dev, c.stream);
    if (selected == 3) return run_cont_pairs<2, 3>(stack, K, npix, sum_mask, part, counts_dev, sums_dev, c.stream);
    return run_cont_pairs<2, 7>(stack, K, npix, sum_mask, part, counts_dev, sums_dev, c.stream);
  });
}
