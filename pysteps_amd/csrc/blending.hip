// Linear and salient blending of nowcasts with NWP on the device (pysteps/blending/linear_blending.py), one lead time
// of all K member pairs per call.  Every pass reads its planes through a host-built table of element offsets
// (nowcast, NWP and result plane of member pair k), so repeated members are never materialised.
//
//  * the load: np.nan_to_num(nwp, nan=0.0) - NaN -> 0, +-inf -> +- the dtype's largest finite value - and the fill of
//    nowcast NaNs with the NWP value cast to the nowcast's dtype (0 without fill_nwp) happen in registers
//  * blend_linear: copy of the filled nowcast (weight 0), copy of the loaded NWP (weight 1), or
//    weight_nwp * nwp + weight_nowcast * nowcast - each product in its array's dtype with the weight rounded to it, the
//    sum in the common dtype, rounded once to the NWP's dtype at the store; contraction is off in this file
//  * the salient lead time: both maxima over the K planes (integer atomicMax on order-preserving keys), then
//    diff = nowcast / max - nwp / max as an order-preserving integer key with -0.0 folded onto 0.0, the dense rank of
//    every key, and ws (the reference's _get_ws in its written order) with the blend in one pass
//  * the dense ranks: an LSD radix sort of the keys alone (radix_sort.h, shared with nqt.hip; 8-bit digits; the histograms of all digits in one read;
//    digits that are constant over the array are skipped; a pass is count -> scan of the (digit, tile) table ->
//    stable scatter, a wave ranks its 64 keys by ballots), first occurrences flagged and compacted to the array of
//    distinct keys, and each pixel's rank is its key's position there by binary search.  Ranks are integers and only
//    integer atomics are used: the same bits in every run.
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "radix_sort.h"

#pragma clang fp contract(off)

namespace psh {
namespace {

constexpr int kMaxGridX = 2048;
constexpr size_t kMaxKeys = static_cast<size_t>(1) << 31;

void *g_ws = nullptr;  // keys, two sort buffers, tables

template <class T> struct Largest;
template <> struct Largest<float> { static __device__ __forceinline__ float value() { return 3.402823466e+38f; } };
template <> struct Largest<double> { static __device__ __forceinline__ double value() { return 1.7976931348623157e+308; } };

template <class T> __device__ __forceinline__ T nan_to_num(T v) {
  if (v != v) return T(0);
  if (v > Largest<T>::value()) return Largest<T>::value();
  if (v < -Largest<T>::value()) return -Largest<T>::value();
  return v;
}

template <class Tn, class Tw> struct Common { using type = double; };
template <> struct Common<float, float> { using type = float; };
template <class C> struct KeyOf { using type = unsigned long long; };
template <> struct KeyOf<float> { using type = unsigned; };

// the planes of one lead time: off[k], off[K + k], off[2 K + k] = element offsets of member pair k's nowcast, NWP and
// result plane
template <class Tn, class Tw> struct Planes {
  const Tn *nc;
  const Tw *nwp;
  Tw *out;
  const long long *off;
  int K;
  size_t plane;
  int fill;
};

struct Small {
  unsigned long long maxkey[2];  // nowcast, NWP
  unsigned distinct;
  int status;  // 1: a maximum is not finite, 2: a diff is NaN
};

template <class Tn, class Tw> __device__ __forceinline__ void load_pair(const Tn *nc, const Tw *nwp, size_t i, int fill, Tn &a, Tw &b) {
  b = nan_to_num(nwp[i]);
  a = nc[i];
  if (a != a) a = fill ? static_cast<Tn>(b) : Tn(0);
}

// MODE 0: the filled nowcast; 1: the loaded NWP (no nowcast plane is read); 2: the weighted sum
template <class Tn, class Tw, int MODE>
__global__ __launch_bounds__(kThreads) void blend_linear(Planes<Tn, Tw> p, double w_nwp, double w_nc) {
  using C = typename Common<Tn, Tw>::type;
  const int k = blockIdx.y;
  const Tn *nc = MODE != 1 ? p.nc + p.off[k] : nullptr;
  const Tw *nwp = p.nwp ? p.nwp + p.off[p.K + k] : nullptr;
  Tw *out = p.out + p.off[2 * p.K + k];
  const Tw wn = static_cast<Tw>(w_nwp);
  const Tn wc = static_cast<Tn>(w_nc);
  const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < p.plane; i += stride) {
    if (MODE == 1) {
      out[i] = nan_to_num(nwp[i]);
    } else if (MODE == 0) {
      Tn a = nc[i];
      if (a != a) a = p.fill ? static_cast<Tn>(nan_to_num(nwp[i])) : Tn(0);
      out[i] = static_cast<Tw>(a);
    } else {
      Tn a;
      Tw b;
      load_pair(nc, nwp, i, p.fill, a, b);
      const Tw p1 = wn * b;
      const Tn p2 = wc * a;
      out[i] = static_cast<Tw>(static_cast<C>(p1) + static_cast<C>(p2));
    }
  }
}

template <class Tn, class Tw> __global__ __launch_bounds__(kThreads) void salient_max(Planes<Tn, Tw> p, Small *small) {
  __shared__ unsigned long long s_max[2];
  if (threadIdx.x < 2) s_max[threadIdx.x] = 0;
  __syncthreads();
  const int k = blockIdx.y;
  const Tn *nc = p.nc + p.off[k];
  const Tw *nwp = p.nwp + p.off[p.K + k];
  unsigned long long ka = 0, kb = 0;
  const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < p.plane; i += stride) {
    Tn a;
    Tw b;
    load_pair(nc, nwp, i, p.fill, a, b);
    ka = max(ka, okey(static_cast<double>(a)));
    kb = max(kb, okey(static_cast<double>(b)));
  }
  atomicMax(&s_max[0], ka);
  atomicMax(&s_max[1], kb);
  __syncthreads();
  if (threadIdx.x < 2) atomicMax(&small->maxkey[threadIdx.x], s_max[threadIdx.x]);
}

template <class Tn, class Tw>
__global__ __launch_bounds__(kThreads) void salient_keys(Planes<Tn, Tw> p, Small *small, typename KeyOf<typename Common<Tn, Tw>::type>::type *keys) {
  using C = typename Common<Tn, Tw>::type;
  const int k = blockIdx.y;
  const Tn *nc = p.nc + p.off[k];
  const Tw *nwp = p.nwp + p.off[p.K + k];
  const double max_a = key_value(small->maxkey[0]), max_b = key_value(small->maxkey[1]);
  const Tn ma = static_cast<Tn>(max_a);  // exact: the maximum is one of the values
  const Tw mb = static_cast<Tw>(max_b);
  int status = (isfinite(max_a) && isfinite(max_b)) ? 0 : 1;
  const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < p.plane; i += stride) {
    Tn a;
    Tw b;
    load_pair(nc, nwp, i, p.fill, a, b);
    const Tn na = ma == Tn(0) ? Tn(0) : a / ma;
    const Tw nb = mb == Tw(0) ? Tw(0) : b / mb;
    const C diff = static_cast<C>(na) - static_cast<C>(nb);
    if (diff != diff) status |= 2;
    keys[static_cast<size_t>(k) * p.plane + i] = okey(diff);
  }
  if (status) atomicOr(&small->status, status);
}

template <class T, class Key> __global__ __launch_bounds__(kThreads) void plain_keys(const T *x, size_t n, Key *keys) {
  const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) keys[i] = okey(x[i]);
}

// ---- distinct keys ----------------------------------------------------------------------------------------------
template <class Key> __global__ __launch_bounds__(kThreads) void heads_count(const Key *sorted, size_t n, size_t per, unsigned *tile_heads) {
  __shared__ unsigned s_total;
  if (threadIdx.x == 0) s_total = 0;
  __syncthreads();
  const size_t t0 = static_cast<size_t>(blockIdx.x) * per, t1 = min(n, t0 + per);
  unsigned c = 0;
  for (size_t i = t0 + threadIdx.x; i < t1; i += kThreads) c += (i == 0 || sorted[i] != sorted[i - 1]) ? 1u : 0u;
  if (c) atomicAdd(&s_total, c);
  __syncthreads();
  if (threadIdx.x == 0) tile_heads[blockIdx.x] = s_total;
}

// one block over the tile table (<= kMaxTiles entries): first place of every tile's distinct keys, and their number
__global__ __launch_bounds__(kThreads) void heads_scan(unsigned *tile_heads, int tiles, unsigned *distinct) {
  constexpr int kPer = kMaxTiles / kThreads;
  __shared__ unsigned s_scan[kThreads];
  const int t = threadIdx.x;
  unsigned v[kPer], sum = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int idx = t * kPer + j;
    v[j] = idx < tiles ? tile_heads[idx] : 0u;
    sum += v[j];
  }
  unsigned total;
  unsigned run = block_exclusive_scan(sum, s_scan, &total);
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int idx = t * kPer + j;
    if (idx < tiles) tile_heads[idx] = run;
    run += v[j];
  }
  if (t == 0) *distinct = total;
}

template <class Key>
__global__ __launch_bounds__(kThreads) void heads_compact(const Key *sorted, size_t n, size_t per, const unsigned *tile_first, Key *uniq) {
  __shared__ unsigned s_wave[kWaves];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const size_t t0 = static_cast<size_t>(blockIdx.x) * per, t1 = min(n, t0 + per);
  size_t carry = tile_first[blockIdx.x];
  const unsigned long long below = (1ull << lane) - 1ull;
  for (size_t base = t0; base < t1; base += kThreads) {
    const size_t i = base + t;
    const bool head = i < t1 && (i == 0 || sorted[i] != sorted[i - 1]);
    const unsigned long long b = __ballot(head);
    if (lane == 0) s_wave[w] = __popcll(b);
    __syncthreads();
    unsigned before = 0, total = 0;
#pragma unroll
    for (int j = 0; j < kWaves; ++j) {
      if (j < w) before += s_wave[j];
      total += s_wave[j];
    }
    __syncthreads();
    const size_t pos = carry + before + __popcll(b & below);
    if (head && pos < n) uniq[pos] = sorted[i];
    carry += total;
  }
}

template <class Key> __device__ __forceinline__ unsigned dense_rank(const Key *uniq, unsigned distinct, Key key) {
  unsigned lo = 0, hi = distinct;
  while (lo < hi) {
    const unsigned mid = lo + ((hi - lo) >> 1);
    if (uniq[mid] < key)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo + 1;
}

template <class Key> __global__ __launch_bounds__(kThreads) void plain_rank(const Key *keys, size_t n, const Key *uniq, const unsigned *distinct, unsigned *rank) {
  const unsigned u = *distinct;
  const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) rank[i] = dense_rank(uniq, u, keys[i]);
}

// rank / U, the reference's _get_ws in its written order (w2 = w ** 2, omw2 = (1 - w) ** 2 from the host), the blend
template <class Tn, class Tw, class Key>
__global__ __launch_bounds__(kThreads) void salient_blend(Planes<Tn, Tw> p, const Key *keys, const Key *uniq, const Small *small, double w,
                                                          double omw, double w2, double omw2) {
  const int k = blockIdx.y;
  const Tn *nc = p.nc + p.off[k];
  const Tw *nwp = p.nwp + p.off[p.K + k];
  Tw *out = p.out + p.off[2 * p.K + k];
  const unsigned distinct = small->distinct;
  const double du = static_cast<double>(distinct);
  const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < p.plane; i += stride) {
    Tn a;
    Tw b;
    load_pair(nc, nwp, i, p.fill, a, b);
    const double rs = static_cast<double>(dense_rank(uniq, distinct, keys[static_cast<size_t>(k) * p.plane + i])) / du;
    const double wr = w * rs;
    const double first = wr / (wr + omw * (1.0 - rs));
    const double s1 = sqrt(rs * rs + w2);
    const double s2 = sqrt((1.0 - rs) * (1.0 - rs) + omw2);
    const double ws = 0.5 * (first + s1 / (s1 + s2));
    out[i] = static_cast<Tw>(ws * static_cast<double>(a) + (1.0 - ws) * static_cast<double>(b));
  }
}

template <class T> __global__ __launch_bounds__(kThreads) void scale_elements(const T *in, T *out, size_t n, T div, T mul) {
  const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) out[i] = in[i] / div * mul;
}

// the cut is decided in dB: r < threshold there is 10^(r/10) < 10^(threshold/10) for a monotone pow, and a pixel at the
// threshold itself stays on the reference's side whatever the last bit of either pow
__global__ __launch_bounds__(kThreads) void db_inverse_f64(const double *in, double *out, size_t n, double threshold_db, double zerovalue) {
  const size_t stride = static_cast<size_t>(gridDim.x) * kThreads;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) {
    const double r = in[i];
    out[i] = r < threshold_db ? zerovalue : pow(10.0, r / 10.0);
  }
}

// ---- host side --------------------------------------------------------------------------------------------------
template <class Key> struct Workspace {
  Key *keys, *buf[2];
  unsigned *ghist, *table, *tile_heads;
  Small *small;
};

template <class Key> int carve(size_t n, Workspace<Key> *w) {
  const size_t key_bytes = align_up(n * sizeof(Key), 256);
  const size_t ghist_bytes = sizeof(Key) * 256 * sizeof(unsigned);
  const size_t table_bytes = static_cast<size_t>(256) * kMaxTiles * sizeof(unsigned);
  const size_t heads_bytes = kMaxTiles * sizeof(unsigned);
  const size_t total = 3 * key_bytes + ghist_bytes + table_bytes + heads_bytes + 256;
  if (int rc = persistent_device(&g_ws, total)) return rc;
  char *base = static_cast<char *>(g_ws);
  w->keys = reinterpret_cast<Key *>(base);
  w->buf[0] = reinterpret_cast<Key *>(base + key_bytes);
  w->buf[1] = reinterpret_cast<Key *>(base + 2 * key_bytes);
  base += 3 * key_bytes;
  w->ghist = reinterpret_cast<unsigned *>(base);
  w->table = reinterpret_cast<unsigned *>(base + ghist_bytes);
  w->tile_heads = reinterpret_cast<unsigned *>(base + ghist_bytes + table_bytes);
  w->small = reinterpret_cast<Small *>(base + ghist_bytes + table_bytes + heads_bytes);
  return PSH_OK;
}

struct StageTimer {
  hipEvent_t ev[5] = {};
  int used = 0;
  bool on = false;
  int start(bool want) {
    on = want;
    if (!on) return PSH_OK;
    for (auto &e : ev) PSH_HIP(hipEventCreate(&e));
    return PSH_OK;
  }
  int mark(hipStream_t s) {
    if (on && used < 5) PSH_HIP(hipEventRecord(ev[used++], s));
    return PSH_OK;
  }
  // ms[0..3]: between consecutive marks; ms[4]: first to last
  int finish(float *ms) {
    if (!on) return PSH_OK;
    int rc = PSH_OK;
    if (used == 5 && hipEventSynchronize(ev[4]) == hipSuccess) {
      for (int j = 0; j < 4; ++j) (void)hipEventElapsedTime(&ms[j], ev[j], ev[j + 1]);
      (void)hipEventElapsedTime(&ms[4], ev[0], ev[4]);
    } else {
      rc = fail(PSH_EHIP, "blend: stage timing failed");
    }
    for (auto &e : ev)
      if (e) (void)hipEventDestroy(e);
    on = false;
    return rc;
  }
};

// keys (n of them, in w.keys) -> *uniq_out: their distinct values in ascending order, w.small->distinct their number.
// ghist_host: the digit histograms of hist_all, already on the host.
template <class Key>
int sort_distinct(const Workspace<Key> &w, size_t n, const unsigned *ghist_host, hipStream_t s, StageTimer *timer, const Key **uniq_out) {
  constexpr int D = sizeof(Key);
  const Tiling tl = tiling(n);
  const Key *src = w.keys;
  int next = 0;
  for (int d = 0; d < D; ++d) {
    bool constant = false;
    for (int j = 0; j < 256; ++j) constant = constant || ghist_host[d * 256 + j] == n;
    if (constant) continue;
    Key *dst = w.buf[next];
    hipLaunchKernelGGL(pass_count<Key>, dim3(tl.tiles), dim3(kThreads), 0, s, src, n, tl.per, 8 * d, w.table);
    hipLaunchKernelGGL(pass_scan, dim3(256), dim3(kThreads), 0, s, w.table, tl.tiles, static_cast<const unsigned *>(w.ghist + d * 256));
    hipLaunchKernelGGL(pass_scatter<Key>, dim3(tl.tiles), dim3(kThreads), 0, s, src, dst, n, tl.per, 8 * d,
                       static_cast<const unsigned *>(w.table));
    src = dst;
    next ^= 1;
  }
  PSH_HIP(hipGetLastError());
  if (int rc = timer->mark(s)) return rc;
  Key *uniq = w.buf[next];  // the buffer the sorted keys are not in
  hipLaunchKernelGGL(heads_count<Key>, dim3(tl.tiles), dim3(kThreads), 0, s, src, n, tl.per, w.tile_heads);
  hipLaunchKernelGGL(heads_scan, dim3(1), dim3(kThreads), 0, s, w.tile_heads, tl.tiles, &w.small->distinct);
  hipLaunchKernelGGL(heads_compact<Key>, dim3(tl.tiles), dim3(kThreads), 0, s, src, n, tl.per, static_cast<const unsigned *>(w.tile_heads), uniq);
  PSH_HIP(hipGetLastError());
  if (int rc = timer->mark(s)) return rc;
  *uniq_out = uniq;
  return PSH_OK;
}

// histograms of every digit in one read, then to the host together with the maxima and the status word
template <class Key> int histograms(const Workspace<Key> &w, size_t n, hipStream_t s, unsigned *ghist_host, Small *small_host) {
  constexpr int D = sizeof(Key);
  const Tiling tl = tiling(n);
  PSH_HIP(hipMemsetAsync(w.ghist, 0, D * 256 * sizeof(unsigned), s));
  hipLaunchKernelGGL(hist_all<Key>, dim3(tl.tiles), dim3(kThreads), 0, s, static_cast<const Key *>(w.keys), n, tl.per, w.ghist);
  PSH_HIP(hipGetLastError());
  PSH_HIP(hipMemcpyAsync(ghist_host, w.ghist, D * 256 * sizeof(unsigned), hipMemcpyDeviceToHost, s));
  PSH_HIP(hipMemcpyAsync(small_host, w.small, sizeof(Small), hipMemcpyDeviceToHost, s));
  PSH_HIP(hipStreamSynchronize(s));
  return PSH_OK;
}

inline unsigned grid_x(size_t n) { return static_cast<unsigned>(std::min<size_t>((n + kThreads - 1) / kThreads, kMaxGridX)); }

template <class Tn, class Tw> int linear_impl(Planes<Tn, Tw> p, int mode, double w_nwp, double w_nc, hipStream_t s) {
  const dim3 grid(grid_x(p.plane), p.K), block(kThreads);
  if (mode == 0)
    hipLaunchKernelGGL((blend_linear<Tn, Tw, 0>), grid, block, 0, s, p, w_nwp, w_nc);
  else if (mode == 1)
    hipLaunchKernelGGL((blend_linear<Tn, Tw, 1>), grid, block, 0, s, p, w_nwp, w_nc);
  else
    hipLaunchKernelGGL((blend_linear<Tn, Tw, 2>), grid, block, 0, s, p, w_nwp, w_nc);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

template <class Tn, class Tw>
int salient_impl(Planes<Tn, Tw> p, double w, double omw, double w2, double omw2, hipStream_t s, int *status, float *stage_ms) {
  using Key = typename KeyOf<typename Common<Tn, Tw>::type>::type;
  const size_t n = static_cast<size_t>(p.K) * p.plane;
  Workspace<Key> ws;
  if (int rc = carve(n, &ws)) return rc;
  StageTimer timer;
  if (int rc = timer.start(stage_ms != nullptr)) return rc;
  if (int rc = timer.mark(s)) return rc;
  const dim3 grid(grid_x(p.plane), p.K), block(kThreads);
  PSH_HIP(hipMemsetAsync(ws.small, 0, sizeof(Small), s));
  hipLaunchKernelGGL((salient_max<Tn, Tw>), grid, block, 0, s, p, ws.small);
  hipLaunchKernelGGL((salient_keys<Tn, Tw>), grid, block, 0, s, p, ws.small, ws.keys);
  PSH_HIP(hipGetLastError());
  unsigned ghist_host[sizeof(Key) * 256];
  Small small_host;
  if (int rc = histograms(ws, n, s, ghist_host, &small_host)) return rc;
  *status = small_host.status;
  if (small_host.status) {
    if (stage_ms) {
      for (int j = 0; j < 4; ++j) (void)timer.mark(s);
      (void)timer.finish(stage_ms);
    }
    return PSH_OK;  // declined: nothing is written
  }
  if (int rc = timer.mark(s)) return rc;
  const Key *uniq = nullptr;
  if (int rc = sort_distinct(ws, n, ghist_host, s, &timer, &uniq)) return rc;
  hipLaunchKernelGGL((salient_blend<Tn, Tw, Key>), grid, block, 0, s, p, static_cast<const Key *>(ws.keys), uniq,
                     static_cast<const Small *>(ws.small), w, omw, w2, omw2);
  PSH_HIP(hipGetLastError());
  if (int rc = timer.mark(s)) return rc;
  return timer.finish(stage_ms);
}

template <class T> int rank_impl(const T *x, size_t n, unsigned *rank, unsigned *distinct_host, hipStream_t s) {
  using Key = typename KeyOf<T>::type;
  Workspace<Key> ws;
  if (int rc = carve(n, &ws)) return rc;
  StageTimer timer;
  PSH_HIP(hipMemsetAsync(ws.small, 0, sizeof(Small), s));
  hipLaunchKernelGGL((plain_keys<T, Key>), dim3(grid_x(n)), dim3(kThreads), 0, s, x, n, ws.keys);
  PSH_HIP(hipGetLastError());
  unsigned ghist_host[sizeof(Key) * 256];
  Small small_host;
  if (int rc = histograms(ws, n, s, ghist_host, &small_host)) return rc;
  const Key *uniq = nullptr;
  if (int rc = sort_distinct(ws, n, ghist_host, s, &timer, &uniq)) return rc;
  hipLaunchKernelGGL(plain_rank<Key>, dim3(grid_x(n)), dim3(kThreads), 0, s, static_cast<const Key *>(ws.keys), n, uniq,
                     static_cast<const unsigned *>(&ws.small->distinct), rank);
  PSH_HIP(hipGetLastError());
  PSH_HIP(hipMemcpyAsync(distinct_host, &ws.small->distinct, sizeof(unsigned), hipMemcpyDeviceToHost, s));
  PSH_HIP(hipStreamSynchronize(s));
  return PSH_OK;
}

int check_planes(const char *what, const void *nwp, const void *out, const void *off, int K, size_t plane) {
  if (!out || !off) return fail(PSH_EINVAL, "%s: NULL pointer", what);
  if (K < 1 || K > 65535 || plane == 0) return fail(PSH_EINVAL, "%s: 1..65535 member pairs, planes not empty", what);
  (void)nwp;
  return PSH_OK;
}

}  // namespace
}  // namespace psh

using psh::fail;

extern "C" int psh_blend_linear_dev(const void *nowcast_dev, int nowcast_f32, const void *nwp_dev, int nwp_f32,
                                    const long long *offsets_dev, int K, size_t plane, int mode, double weight_nwp,
                                    double weight_nowcast, int fill_nwp, void *out_dev) {
  PSH_ENTER(c);
  if (int rc = psh::check_planes("blend_linear", nwp_dev, out_dev, offsets_dev, K, plane)) return rc;
  if (mode < 0 || mode > 2) return fail(PSH_EINVAL, "blend_linear: mode must be 0, 1 or 2");
  if (mode != 1 && !nowcast_dev) return fail(PSH_EINVAL, "blend_linear: the nowcast is needed");
  if ((mode != 0 || fill_nwp) && !nwp_dev) return fail(PSH_EINVAL, "blend_linear: the NWP is needed");
#define PSH_BLEND_LINEAR(TN, TW)                                                                                          \
  return psh::linear_impl(psh::Planes<TN, TW>{static_cast<const TN *>(nowcast_dev), static_cast<const TW *>(nwp_dev),   \
                                              static_cast<TW *>(out_dev), offsets_dev, K, plane, fill_nwp},               \
                          mode, weight_nwp, weight_nowcast, c.stream)
  if (nowcast_f32 && nwp_f32) PSH_BLEND_LINEAR(float, float);
  if (nowcast_f32) PSH_BLEND_LINEAR(float, double);
  if (nwp_f32) PSH_BLEND_LINEAR(double, float);
  PSH_BLEND_LINEAR(double, double);
#undef PSH_BLEND_LINEAR
}

extern "C" int psh_blend_salient_dev(const void *nowcast_dev, int nowcast_f32, const void *nwp_dev, int nwp_f32,
                                     const long long *offsets_dev, int K, size_t plane, double weight, double one_minus_weight,
                                     double weight_sq, double one_minus_weight_sq, int fill_nwp, void *out_dev, int *status,
                                     float *stage_ms) {
  PSH_ENTER(c);
  if (int rc = psh::check_planes("blend_salient", nwp_dev, out_dev, offsets_dev, K, plane)) return rc;
  if (!nowcast_dev || !nwp_dev || !status) return fail(PSH_EINVAL, "blend_salient: NULL pointer");
  if (plane > psh::kMaxKeys / static_cast<size_t>(K)) return fail(PSH_EUNSUPPORTED, "blend_salient: more than 2^31 values to rank");
#define PSH_BLEND_SALIENT(TN, TW)                                                                                          \
  return psh::salient_impl(psh::Planes<TN, TW>{static_cast<const TN *>(nowcast_dev), static_cast<const TW *>(nwp_dev),   \
                                               static_cast<TW *>(out_dev), offsets_dev, K, plane, fill_nwp},               \
                           weight, one_minus_weight, weight_sq, one_minus_weight_sq, c.stream, status, stage_ms)
  if (nowcast_f32 && nwp_f32) PSH_BLEND_SALIENT(float, float);
  if (nowcast_f32) PSH_BLEND_SALIENT(float, double);
  if (nwp_f32) PSH_BLEND_SALIENT(double, float);
  PSH_BLEND_SALIENT(double, double);
#undef PSH_BLEND_SALIENT
}

extern "C" int psh_blend_dense_rank_dev(const void *x_dev, int f32, size_t n, unsigned *rank_dev, unsigned *distinct) {
  PSH_ENTER(c);
  if (!x_dev || !rank_dev || !distinct) return fail(PSH_EINVAL, "blend_dense_rank: NULL pointer");
  if (n == 0) return fail(PSH_EINVAL, "blend_dense_rank: nothing to rank");
  if (n > psh::kMaxKeys) return fail(PSH_EUNSUPPORTED, "blend_dense_rank: more than 2^31 values to rank");
  return psh::with_real(x_dev, !f32, [&](auto *x) { return psh::rank_impl(x, n, rank_dev, distinct, c.stream); });
}

extern "C" int psh_blend_db_inverse_f64_dev(const double *in_dev, double *out_dev, size_t n, double threshold_db, double zerovalue) {
  PSH_ENTER(c);
  if (n == 0) return PSH_OK;
  if (!in_dev || !out_dev) return fail(PSH_EINVAL, "blend_db_inverse_f64: NULL pointer");
  hipLaunchKernelGGL(psh::db_inverse_f64, dim3(psh::grid_x(n)), dim3(psh::kThreads), 0, c.stream, in_dev, out_dev, n, threshold_db, zerovalue);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

extern "C" int psh_blend_scale_dev(const void *in_dev, void *out_dev, int f32, size_t n, double divisor, double factor) {
  PSH_ENTER(c);
  if (n == 0) return PSH_OK;
  if (!in_dev || !out_dev) return fail(PSH_EINVAL, "blend_scale: NULL pointer");
  const dim3 grid(psh::grid_x(n)), block(psh::kThreads);
  if (f32)
    hipLaunchKernelGGL(psh::scale_elements<float>, grid, block, 0, c.stream, static_cast<const float *>(in_dev), static_cast<float *>(out_dev),
                       n, static_cast<float>(divisor), static_cast<float>(factor));
  else
    hipLaunchKernelGGL(psh::scale_elements<double>, grid, block, 0, c.stream, static_cast<const double *>(in_dev),
                       static_cast<double *>(out_dev), n, divisor, factor);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}
