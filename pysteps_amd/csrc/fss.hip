// The fractions skill score (pysteps/verification/spatialscores.py fss_accum, Roberts and Lean 2008) on gfx950: the
// three sums behind the score, for a stack of forecasts against one observation or a stack of them, for several
// thresholds and several scales in one call.
//
// The reference turns both fields into 0/1 maps (finite and >= threshold), averages each with
// scipy.ndimage.uniform_filter(size = s, mode = "constant", cval = 0) and sums S_f^2, S_f S_o and S_o^2 over the
// image.  S = c / s^2 with c the number of ones in the window, rows y - s/2 .. y - s/2 + s - 1 and the same columns,
// clipped to the image, so the three sums are sum(c_f^2), sum(c_f c_o) and sum(c_o^2) over s^4: integers.  The kernels
// count them and return the integers; the caller divides once.
//   fss_prefix_*   per row the prefix counts of both maps, forecast in the low and observation in the high half of one
//                  uint32, rows of n + 1 words with a leading zero (the scan of row_prefix.h, shared with lagprob.hip).
//                  An observation shared by all forecasts is scanned once (fss_prefix_obs) and its words are taken over
//                  by the members' rows (fss_prefix_member).
//   fss_box        a thread owns one column of a band of rows, for 8, 4, 2 or 1 scales at a time.  The horizontal count of
//                  a row is one packed difference of two prefix words; the vertical sum over the s rows of the window
//                  is a running sum down the column (add the entering row, subtract the leaving one), started from
//                  the s rows around the band's first row, so the cost per pixel does not grow with s.  Packed sums
//                  are plain uint32 arithmetic: both halves end below 65536 (s <= 255), so what a transient carry
//                  moves between the halves comes back.  The products (< 2^32) are accumulated in 64-bit integers in
//                  registers, reduced over the wave by shuffles and over the workgroup through LDS; one
//                  atomicAdd(unsigned long long) per sum and workgroup.  Integer adds commute: the result does not
//                  depend on the order of arrival.
// Range: s <= 255 and n <= 65535 keep a count within 16 bits; with m <= 65535 as well a sum stays below 2^64.
#include "common.h"
#include "row_prefix.h"

namespace psh {
namespace {

constexpr int kFssMaxScale = 255;
constexpr int kFssMaxDim = kPackedPrefixMaxWidth;
constexpr int kFssThreads = 256;
constexpr size_t kFssPrefixBytes = size_t(256) << 20;  // prefix planes of the members of one batch
constexpr int kFssTargetGroups = 2048;               // workgroups of a box launch the band height aims at

enum { kFssPair = 0, kFssMember = 1, kFssObs = 2 };  // which sums a box launch adds: all, ff and fo, oo

template <typename T>
__device__ __forceinline__ uint32_t above(T x, double thr) {
  return (__builtin_isfinite(x) && static_cast<double>(x) >= thr) ? 1u : 0u;
}

// grid (m, members of the batch); fct / obs point at the batch's first plane
template <typename TF, typename TO>
__global__ __launch_bounds__(kFssThreads) void fss_prefix_pair(const TF *__restrict__ fct, const TO *__restrict__ obs, int n,
                                                                double thr_f, double thr_o, uint32_t *__restrict__ prefix) {
  __shared__ uint32_t wave_sum[kFssThreads / 64];
  const size_t row = static_cast<size_t>(blockIdx.y) * gridDim.x + blockIdx.x;
  const TF *f = fct + row * n;
  const TO *o = obs + row * n;
  packed_row_prefix<kFssThreads>(n, prefix + row * (static_cast<size_t>(n) + 1), wave_sum,
                                 [&](int x) { return above(f[x], thr_f) | (above(o[x], thr_o) << 16); });
}

template <typename TF>
__global__ __launch_bounds__(kFssThreads) void fss_prefix_member(const TF *__restrict__ fct, const uint32_t *__restrict__ obs_prefix,
                                                                  int n, double thr_f, uint32_t *__restrict__ prefix) {
  __shared__ uint32_t wave_sum[kFssThreads / 64];
  const size_t row = static_cast<size_t>(blockIdx.y) * gridDim.x + blockIdx.x;
  const TF *f = fct + row * n;
  const uint32_t *o = obs_prefix + blockIdx.x * (static_cast<size_t>(n) + 1);  // low halves are zero
  packed_row_prefix<kFssThreads>(n, prefix + row * (static_cast<size_t>(n) + 1), wave_sum,
                                 [&](int x) { return above(f[x], thr_f) | (o[x + 1] - o[x]); });
}

template <typename TO>
__global__ __launch_bounds__(kFssThreads) void fss_prefix_obs(const TO *__restrict__ obs, int n, double thr_o,
                                                               uint32_t *__restrict__ obs_prefix) {
  __shared__ uint32_t wave_sum[kFssThreads / 64];
  const size_t row = blockIdx.x;
  const TO *o = obs + row * n;
  packed_row_prefix<kFssThreads>(n, obs_prefix + row * (static_cast<size_t>(n) + 1), wave_sum,
                                 [&](int x) { return above(o[x], thr_o) << 16; });
}

template <int NS>
struct FssScales {
  int s[NS];  // 1 .. 255
};

// grid (ceil(n / 256), ceil(m / band), members of the batch); out points at the first member's first sum of this pass
template <int NS, int MODE>
__global__ __launch_bounds__(kFssThreads) void fss_box(const uint32_t *__restrict__ prefix, int m, int n, int band,
                                                        FssScales<NS> sc, unsigned long long *__restrict__ out,
                                                        size_t out_member_stride) {
  __shared__ unsigned long long red[kFssThreads / 64][NS * 3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int x = blockIdx.x * kFssThreads + tid;
  const int y0 = blockIdx.y * band, y1 = min(y0 + band, m);
  const size_t pitch = static_cast<size_t>(n) + 1;
  const uint32_t *P = prefix + static_cast<size_t>(blockIdx.z) * m * pitch;

  // window of scale s: rows / columns -a .. +b around the pixel; prefix columns lo (exclusive start) and hi, both in
  // [0, n]; a lane beyond the image reads column n twice and counts nothing
  int lo[NS], hi[NS], amax = 0, bmax = 0;
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const int a = sc.s[j] / 2, b = sc.s[j] - 1 - a;
    lo[j] = x < n ? max(x - a, 0) : n;
    hi[j] = x < n ? min(x + b + 1, n) : n;
    amax = max(amax, a);
    bmax = max(bmax, b);
  }

  uint32_t V[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) V[j] = 0u;
  for (int r = max(y0 - amax, 0); r <= min(y0 + bmax, m - 1); ++r) {
    const uint32_t *row = P + r * pitch;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      const int a = sc.s[j] / 2, b = sc.s[j] - 1 - a;
      if (r >= y0 - a && r <= y0 + b) {
        PSH_DASSERT(lo[j] >= 0 && lo[j] <= hi[j] && hi[j] <= n);
        V[j] += row[hi[j]] - row[lo[j]];
      }
    }
  }

  unsigned long long acc[NS][3];
#pragma unroll
  for (int j = 0; j < NS; ++j) acc[j][0] = acc[j][1] = acc[j][2] = 0ull;

  for (int y = y0; y < y1; ++y) {
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      const unsigned long long cf = V[j] & 0xffffu, co = V[j] >> 16;
      if (MODE != kFssObs) {
        acc[j][0] += cf * cf;
        acc[j][1] += cf * co;
      }
      if (MODE != kFssMember) acc[j][2] += co * co;
    }
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      const int a = sc.s[j] / 2, b = sc.s[j] - 1 - a;
      const int enter = y + 1 + b, leave = y - a;
      if (enter < m) {
        const uint32_t *row = P + enter * pitch;
        V[j] += row[hi[j]] - row[lo[j]];
      }
      if (leave >= 0) {
        const uint32_t *row = P + leave * pitch;
        V[j] -= row[hi[j]] - row[lo[j]];
      }
    }
  }

#pragma unroll
  for (int j = 0; j < NS; ++j) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if ((MODE == kFssObs && c != 2) || (MODE == kFssMember && c == 2)) continue;
      unsigned long long v = acc[j][c];
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
      if (lane == 0) red[wave][j * 3 + c] = v;
    }
  }
  __syncthreads();
  if (tid < NS * 3) {
    const int c = tid % 3;
    if ((MODE == kFssObs && c != 2) || (MODE == kFssMember && c == 2)) return;
    unsigned long long v = 0ull;
#pragma unroll
    for (int w = 0; w < kFssThreads / 64; ++w) v += red[w][tid];
    atomicAdd(out + blockIdx.z * out_member_stride + tid, v);
  }
}

// a shared observation: sum(c_o^2) was counted once, into member 0
__global__ void fss_spread_obs(unsigned long long *__restrict__ out, int K, int per_member) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (K - 1) * per_member) return;
  const int k = 1 + i / per_member, e = i % per_member;
  out[(static_cast<size_t>(k) * per_member + e) * 3 + 2] = out[static_cast<size_t>(e) * 3 + 2];
}

int band_height(int m, int n, int members, int smax) {
  const long long groups_per_row = static_cast<long long>((n + kFssThreads - 1) / kFssThreads) * members;
  // a band walks band + s rows: not much below s; not so tall that the launch leaves the chip idle
  const long long fill = static_cast<long long>(m) * groups_per_row / kFssTargetGroups;
  const int floor_rows = smax < 32 ? 32 : (smax > 128 ? 128 : smax);
  return static_cast<int>(fill < floor_rows ? floor_rows : (fill > 256 ? 256 : fill));
}

template <int NS, int MODE>
int launch_box(const uint32_t *prefix, int m, int n, int members, const int *scales, unsigned long long *out, size_t stride,
               hipStream_t s) {
  FssScales<NS> sc;
  int smax = 1;
  for (int j = 0; j < NS; ++j) {
    sc.s[j] = scales[j];
    smax = scales[j] > smax ? scales[j] : smax;
  }
  const int band = band_height(m, n, members, smax);
  const dim3 grid((n + kFssThreads - 1) / kFssThreads, (m + band - 1) / band, members);
  hipLaunchKernelGGL((fss_box<NS, MODE>), grid, dim3(kFssThreads), 0, s, prefix, m, n, band, sc, out, stride);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

// all scales of one threshold: passes of 8, 4, 2 and 1 scales; out points at scale 0 of the first member
template <int MODE>
int box_passes(const uint32_t *prefix, int m, int n, int members, const int *scales, int nsc, unsigned long long *out,
               size_t stride, hipStream_t s) {
  int j = 0;
  while (j < nsc) {
    const int left = nsc - j;
    int rc;
    if (left >= 8) {
      rc = launch_box<8, MODE>(prefix, m, n, members, scales + j, out + j * 3, stride, s);
      j += 8;
    } else if (left >= 4) {
      rc = launch_box<4, MODE>(prefix, m, n, members, scales + j, out + j * 3, stride, s);
      j += 4;
    } else if (left >= 2) {
      rc = launch_box<2, MODE>(prefix, m, n, members, scales + j, out + j * 3, stride, s);
      j += 2;
    } else {
      rc = launch_box<1, MODE>(prefix, m, n, members, scales + j, out + j * 3, stride, s);
      j += 1;
    }
    if (rc) return rc;
  }
  return PSH_OK;
}

struct FssCall {
  int K, m, n, nthr, nsc, obs_shared;
  const double *thr_f, *thr_o;
  const int *scales;
  uint32_t *prefix, *obs_prefix;
  int batch;
  unsigned long long *out;
};

template <typename TF, typename TO>
int run(const FssCall &c, const TF *fct, const TO *obs, hipStream_t s) {
  const size_t plane = static_cast<size_t>(c.m) * c.n;
  const size_t stride = static_cast<size_t>(c.nthr) * c.nsc * 3;
  for (int t = 0; t < c.nthr; ++t) {
    unsigned long long *out_t = c.out + static_cast<size_t>(t) * c.nsc * 3;
    if (c.obs_shared) {
      hipLaunchKernelGGL(fss_prefix_obs<TO>, dim3(c.m), dim3(kFssThreads), 0, s, obs, c.n, c.thr_o[t], c.obs_prefix);
      PSH_HIP(hipGetLastError());
      if (int rc = box_passes<kFssObs>(c.obs_prefix, c.m, c.n, 1, c.scales, c.nsc, out_t, stride, s)) return rc;
    }
    for (int k0 = 0; k0 < c.K; k0 += c.batch) {
      const int members = c.K - k0 < c.batch ? c.K - k0 : c.batch;
      const TF *f = fct + k0 * plane;
      unsigned long long *out_k = out_t + k0 * stride;
      if (c.obs_shared) {
        hipLaunchKernelGGL(fss_prefix_member<TF>, dim3(c.m, members), dim3(kFssThreads), 0, s, f,
                           static_cast<const uint32_t *>(c.obs_prefix), c.n, c.thr_f[t], c.prefix);
        PSH_HIP(hipGetLastError());
        if (int rc = box_passes<kFssMember>(c.prefix, c.m, c.n, members, c.scales, c.nsc, out_k, stride, s)) return rc;
      } else {
        hipLaunchKernelGGL((fss_prefix_pair<TF, TO>), dim3(c.m, members), dim3(kFssThreads), 0, s, f, obs + k0 * plane, c.n,
                           c.thr_f[t], c.thr_o[t], c.prefix);
        PSH_HIP(hipGetLastError());
        if (int rc = box_passes<kFssPair>(c.prefix, c.m, c.n, members, c.scales, c.nsc, out_k, stride, s)) return rc;
      }
    }
  }
  if (c.obs_shared && c.K > 1) {
    const int per_member = c.nthr * c.nsc, total = (c.K - 1) * per_member;
    hipLaunchKernelGGL(fss_spread_obs, dim3((total + 255) / 256), dim3(256), 0, s, c.out, c.K, per_member);
    PSH_HIP(hipGetLastError());
  }
  return PSH_OK;
}

}  // namespace
}  // namespace psh

using psh::fail;

extern "C" int psh_fss_sums_dev(const void *fct_dev, int fct_f64, const void *obs_dev, int obs_f64, int obs_shared, int K,
                                int m, int n, const double *thr_fct_host, const double *thr_obs_host, int n_thresholds,
                                const double *scales_host, int n_scales, unsigned long long *out_dev) {
  using namespace psh;
  PSH_ENTER(c);
  if (!fct_dev || !obs_dev || !thr_fct_host || !thr_obs_host || !scales_host || !out_dev) return fail(PSH_EINVAL, "fss: NULL pointer");
  if (m < 1 || n < 1) return fail(PSH_EINVAL, "fss: invalid shape (%d,%d)", m, n);
  if (m > kFssMaxDim || n > kFssMaxDim) return fail(PSH_EUNSUPPORTED, "fss: shape (%d,%d) (at most %d each way)", m, n, kFssMaxDim);
  if (K < 1 || K > 65535) return fail(PSH_EINVAL, "fss: %d forecasts (1..65535)", K);
  if (n_thresholds < 1 || n_thresholds > 4096 || n_scales < 1 || n_scales > 4096)
    return fail(PSH_EINVAL, "fss: %d thresholds, %d scales (1..4096 each)", n_thresholds, n_scales);
  int scales[4096];
  for (int j = 0; j < n_scales; ++j) {
    const double s = scales_host[j];
    if (!(s > 1.0)) {
      scales[j] = 1;  // the reference filters for scale > 1 only: the 0/1 maps themselves
    } else if (s > kFssMaxScale || s != std::floor(s)) {
      return fail(PSH_EUNSUPPORTED, "fss: scale %g (an integer up to %d)", s, kFssMaxScale);
    } else {
      scales[j] = static_cast<int>(s);
    }
  }
  const size_t plane_bytes = static_cast<size_t>(m) * (static_cast<size_t>(n) + 1) * sizeof(uint32_t);
  size_t batch = kFssPrefixBytes / plane_bytes;
  batch = batch < 1 ? 1 : (batch > static_cast<size_t>(K) ? K : batch);
  psh::Scratch blk;
  if (int rc = blk.alloc(plane_bytes * (batch + (obs_shared ? 1 : 0)))) return rc;
  FssCall call;
  call.K = K, call.m = m, call.n = n, call.nthr = n_thresholds, call.nsc = n_scales, call.obs_shared = obs_shared ? 1 : 0;
  call.thr_f = thr_fct_host, call.thr_o = thr_obs_host, call.scales = scales;
  call.prefix = blk.as<uint32_t>();
  call.obs_prefix = call.prefix + batch * (plane_bytes / sizeof(uint32_t));
  call.batch = static_cast<int>(batch);
  call.out = out_dev;
  PSH_HIP(hipMemsetAsync(out_dev, 0, static_cast<size_t>(K) * n_thresholds * n_scales * 3 * sizeof(unsigned long long), c.stream));
  return with_real(fct_dev, fct_f64 != 0, [&](auto *fct) {
    return with_real(obs_dev, obs_f64 != 0, [&](auto *obs) { return run(call, fct, obs, c.stream); });
  });
}
