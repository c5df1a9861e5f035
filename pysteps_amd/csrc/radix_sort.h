// Key-only LSD radix sort shared by blending.hip (dense ranks) and nqt.hip (normal-quantile transform): order-preserving
// integer keys of float32 / float64 values and the three kernels of one 8-bit pass.  A pass is count -> scan of the
// (digit, tile) table -> stable scatter; a wave ranks its 64 keys by ballots.  hist_all gives the histograms of all
// digits in one read, so that the caller can skip digits that are constant over the array.  Only integer atomics:
// the same bits in every run.  Everything lives in the including file's unnamed namespace.
#pragma once

#include <algorithm>

#include "common.h"

namespace psh {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxTiles = 2048;     // tiles of the sort: the (digit, tile) table has 256 x this many entries at most
constexpr size_t kMinTile = 2048;   // keys per tile from which the tile count grows

// order-preserving integer image; -0.0 and 0.0 share one key
__device__ __forceinline__ unsigned okey(float x) {
  const unsigned b = __float_as_uint(x == 0.0f ? 0.0f : x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ unsigned long long okey(double x) {
  const unsigned long long b = static_cast<unsigned long long>(__double_as_longlong(x == 0.0 ? 0.0 : x));
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_value(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double(static_cast<long long>(b));
}

// tile b holds keys [b per, min(n, (b + 1) per)); per is a multiple of kThreads

__device__ __forceinline__ bool wave_uniform(unsigned v, bool valid) {
  const unsigned first = __builtin_amdgcn_readfirstlane(v);
  return __all(valid && v == first);
}

// one more count in bin `bin` of an LDS histogram; a wave whose 64 keys share the bin - the dry area - adds 64 once
__device__ __forceinline__ void hist_add(unsigned *hist, unsigned bin, bool valid) {
  if (wave_uniform(bin, valid)) {
    if ((threadIdx.x & 63) == 0) atomicAdd(&hist[bin], 64u);
  } else if (valid) {
    atomicAdd(&hist[bin], 1u);
  }
}

template <class Key> __global__ __launch_bounds__(kThreads) void hist_all(const Key *keys, size_t n, size_t per, unsigned *ghist) {
  constexpr int D = sizeof(Key);
  __shared__ unsigned s_hist[D * 256];
  for (int j = threadIdx.x; j < D * 256; j += kThreads) s_hist[j] = 0;
  __syncthreads();
  const size_t t0 = static_cast<size_t>(blockIdx.x) * per, t1 = min(n, t0 + per);
  for (size_t base = t0; base < t1; base += kThreads) {  // whole waves take every round: hist_add votes
    const size_t i = base + threadIdx.x;
    const bool valid = i < t1;
    const Key key = valid ? keys[i] : Key(0);
#pragma unroll
    for (int d = 0; d < D; ++d) hist_add(s_hist + d * 256, static_cast<unsigned>(key >> (8 * d)) & 255u, valid);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < D * 256; j += kThreads)
    if (s_hist[j]) atomicAdd(&ghist[j], s_hist[j]);
}

// table[digit * tiles + tile] = keys of the tile with that digit
template <class Key> __global__ __launch_bounds__(kThreads) void pass_count(const Key *keys, size_t n, size_t per, int shift, unsigned *table) {
  __shared__ unsigned s_hist[256];
  s_hist[threadIdx.x] = 0;
  __syncthreads();
  const size_t t0 = static_cast<size_t>(blockIdx.x) * per, t1 = min(n, t0 + per);
  for (size_t base = t0; base < t1; base += kThreads) {
    const size_t i = base + threadIdx.x;
    const bool valid = i < t1;
    const Key key = valid ? keys[i] : Key(0);
    hist_add(s_hist, static_cast<unsigned>(key >> shift) & 255u, valid);
  }
  __syncthreads();
  table[static_cast<size_t>(threadIdx.x) * gridDim.x + blockIdx.x] = s_hist[threadIdx.x];
}

// exclusive scan over kThreads values, one per thread; *total = their sum
__device__ __forceinline__ unsigned block_exclusive_scan(unsigned v, unsigned *s_scan, unsigned *total) {
  const int t = threadIdx.x;
  s_scan[t] = v;
  __syncthreads();
  for (int off = 1; off < kThreads; off <<= 1) {
    const unsigned add = t >= off ? s_scan[t - off] : 0u;
    __syncthreads();
    s_scan[t] += add;
    __syncthreads();
  }
  const unsigned incl = s_scan[t];
  *total = s_scan[kThreads - 1];
  __syncthreads();
  return incl - v;
}

// block d: row d of the table becomes the first position of digit d's keys of every tile; tiles <= kMaxTiles
__global__ __launch_bounds__(kThreads) void pass_scan(unsigned *table, int tiles, const unsigned *digit_hist) {
  constexpr int kPer = kMaxTiles / kThreads;
  __shared__ unsigned s_scan[kThreads];
  const int d = blockIdx.x, t = threadIdx.x;
  unsigned below;
  (void)block_exclusive_scan(t < d ? digit_hist[t] : 0u, s_scan, &below);
  unsigned *row = table + static_cast<size_t>(d) * tiles;
  unsigned v[kPer], sum = 0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int idx = t * kPer + j;
    v[j] = idx < tiles ? row[idx] : 0u;
    sum += v[j];
  }
  unsigned total;
  unsigned run = below + block_exclusive_scan(sum, s_scan, &total);
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const int idx = t * kPer + j;
    if (idx < tiles) row[idx] = run;
    run += v[j];
  }
}

// stable: wave w takes the w-th quarter of the tile in order, 64 keys a round; keys of a round with the same digit
// find each other by ballots and take consecutive places from the wave's counter of that digit
template <class Key>
__global__ __launch_bounds__(kThreads) void pass_scatter(const Key *src, Key *dst, size_t n, size_t per, int shift, const unsigned *table) {
  __shared__ unsigned s_cnt[kWaves][256];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  for (int j = 0; j < kWaves; ++j) s_cnt[j][t] = 0;
  __syncthreads();
  const size_t t0 = static_cast<size_t>(blockIdx.x) * per, t1 = min(n, t0 + per);
  const size_t wlen = per / kWaves;  // a multiple of 64
  const size_t w0 = min(t1, t0 + w * wlen), w1 = min(t1, w0 + wlen);
  for (size_t base = w0; base < w1; base += 64) {
    const size_t i = base + lane;
    const bool valid = i < w1;
    const Key key = valid ? src[i] : Key(0);
    hist_add(s_cnt[w], static_cast<unsigned>(key >> shift) & 255u, valid);
  }
  __syncthreads();
  {
    unsigned run = table[static_cast<size_t>(t) * gridDim.x + blockIdx.x];
    for (int j = 0; j < kWaves; ++j) {
      const unsigned c = s_cnt[j][t];
      s_cnt[j][t] = run;
      run += c;
    }
  }
  __syncthreads();
  volatile unsigned *cnt = s_cnt[w];
  const unsigned long long below = (1ull << lane) - 1ull;
  for (size_t base = w0; base < w1; base += 64) {
    const size_t i = base + lane;
    const bool valid = i < w1;
    const Key key = valid ? src[i] : Key(0);
    const unsigned digit = static_cast<unsigned>(key >> shift) & 255u;
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool set = (digit >> bit) & 1u;
      const unsigned long long m = __ballot(valid && set);
      peers &= set ? m : ~m;
    }
    const unsigned rank = __popcll(peers & below);
    const unsigned first = cnt[digit];
    __builtin_amdgcn_wave_barrier();
    if (valid && rank == 0) cnt[digit] = first + __popcll(peers);
    __builtin_amdgcn_wave_barrier();
    const size_t pos = static_cast<size_t>(first) + rank;
    if (valid && pos < n) dst[pos] = key;
  }
}

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct Tiling {
  size_t per;
  int tiles;
};
inline Tiling tiling(size_t n) {
  size_t per = std::max(kMinTile, align_up((n + kMaxTiles - 1) / kMaxTiles, kThreads));
  return Tiling{per, static_cast<int>((n + per - 1) / per)};
}

}  // namespace
}  // namespace psh
