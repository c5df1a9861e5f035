// Dense-image front end of Lucas-Kanade for gfx950: frame cleaning, uint8
// quantisation, Shi-Tomasi corner response / selection, Gaussian pyramid, Scharr
// gradients and the pyramidal LK tracker.
//
// Replaces the NumPy + OpenCV stages of pysteps/motion/lucaskanade.py:205-242:
//   pysteps/utils/images.py:58-86            morph_opening  (cv2.morphologyEx OPEN, 3x3 cross)
//   pysteps/feature/shitomasi.py:122-171     mask buffering, uint8 rescale, cv2.goodFeaturesToTrack
//   pysteps/tracking/lucaskanade.py:130-189  uint8 rescale, cv2.calcOpticalFlowPyrLK
// OpenCV is a third-party dependency that is not part of the reference tree; the
// kernels follow the published OpenCV 4.x algorithms as restated in
// oracle/lk_opencv.py (cornerMinEigenVal, goodFeaturesToTrack, pyrDown,
// calcSharrDeriv, LKTrackerInvoker) - see the notes there and in DESIGN.md.
//
// All image passes are HBM-streaming stencils (LDS-staged halos, coalesced rows);
// reductions are two-stage (per-block partials + one finishing block), so results
// are deterministic and no statistic ever travels to the host between kernels.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <vector>

#include "common.h"

#pragma clang fp contract(off)

namespace psh {
namespace {

// ---- device-side statistics block (floats) ---------------------------------
enum Stat : int {
  kMinAll = 0,   // min over finite pixels of the raw frame (= fill value)
  kNanCount,     // number of non-finite pixels (as float; exact below 2^24, >0 is what matters)
  kMaxAll,       // max over finite pixels after opening
  kMinFeat,      // min / max over finite pixels of rows >= first usable row (shitomasi.py:140 quirk)
  kMaxFeat,
  kEigMax,       // max corner response over allowed pixels
  kNumStats = 8
};

constexpr int kRedBlocks = 1024;

// Statistics without a finishing launch.  A producing pass used to write one partial per workgroup and
// a single-workgroup kernel folded them (5 such launches per frame pair, 6-12 us each, 255 compute
// units idle).  Minimum and maximum do not depend on the order they are taken in, so a workgroup now
// folds its partial into one of kSlots words with a device-scope atomic (a single word would take the
// ~90 atomics per microsecond one address sustains; 64 words take them side by side), and every
// wave of the CONSUMING pass reads the 64 words back and reduces them itself - the kernel boundary in
// between orders the two.  Floats are kept as order-preserving unsigned keys; minima as the complement
// of the key, so that every word is a maximum and zero-filled memory is the identity.
constexpr int kSlots = 64;
// (kSlCand: word 0 = number of corner candidates, word 1 = workgroups of the fused response pass that are done)
enum SlotKind : int { kSlMin = 0, kSlNan, kSlMaxAll, kSlMinFeat, kSlMaxFeat, kSlEig, kSlCand, kSlotKinds };
constexpr size_t kSlotBytes = sizeof(unsigned) * kSlots * kSlotKinds;  // per frame; cleared before the first pass

__device__ __forceinline__ unsigned float_key(float f) {
  const unsigned b = __float_as_uint(f);
  return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_float(unsigned k) {
  return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ void slot_max(unsigned *slots, int kind, int block, float v) {
  atomicMax(&slots[kind * kSlots + (block & (kSlots - 1))], float_key(v));
}
__device__ __forceinline__ void slot_min(unsigned *slots, int kind, int block, float v) {
  atomicMax(&slots[kind * kSlots + (block & (kSlots - 1))], ~float_key(v));
}

// Row band of a frame that is processed as a sub-image (multi-GPU tiling, lk_band.hip): the
// kernels run on the rows [y_org, y_org + m) of the full frame through an offset pointer; y_org
// restores the absolute row index where the reference's semantics depend on it (the row 0 / 1 quirk
// of shitomasi.py:140, pixel addresses of corner candidates), [lo, hi) are the sub-image rows that
// contribute to statistics / candidates (the rows this rank owns; the rest is halo).  The whole
// frame is {0, 0, m}.
struct Band {
  int y_org, lo, hi;
};

__device__ __forceinline__ int reflect101(int i, int n) {
  if (n == 1) return 0;
  if (i < 0) i = -i;
  if (i >= n) {
    const int period = 2 * (n - 1);
    i %= period;
    if (i >= n) i = period - i;
  }
  return i;
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = fminf(v, __shfl_xor(v, d));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned o = static_cast<unsigned>(__shfl_xor(static_cast<int>(v), d));
    v = o > v ? o : v;
  }
  return v;
}
// every lane of a wave gets the statistic folded into the 64 words of `kind` (lane = word)
__device__ __forceinline__ float slots_max(const unsigned *slots, int kind) {
  return key_float(wave_max_u32(slots[kind * kSlots + (threadIdx.x & 63)]));
}
__device__ __forceinline__ float slots_min(const unsigned *slots, int kind) {
  return key_float(~wave_max_u32(slots[kind * kSlots + (threadIdx.x & 63)]));
}
__device__ __forceinline__ float slots_count(const unsigned *slots, int kind) {  // sum of the words
  unsigned v = slots[kind * kSlots + (threadIdx.x & 63)];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += static_cast<unsigned>(__shfl_xor(static_cast<int>(v), d));
  return static_cast<float>(v);
}

// v_max_f32 / v_min_f32 as they are, for operands that are known not to be NaN (fmaxf / fminf put a
// canonicalising instruction in front of every operand that was selected or loaded)
__device__ __forceinline__ float max_plain(float a, float b) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float min_plain(float a, float b) {
  float r;
  asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// block-wide reductions for the single-block finishing kernels (up to 16 waves)
constexpr int kFinalThreads = 1024;
enum class Red { kMin, kMax, kSum };
template <Red OP>
__device__ __forceinline__ float block_reduce(float v, float *smem /* [16] */) {
  v = OP == Red::kMin ? wave_min(v) : OP == Red::kMax ? wave_max(v) : wave_sum(v);
  const int wave = threadIdx.x >> 6, nwaves = (blockDim.x + 63) >> 6;
  __syncthreads();  // smem may still be read from a previous reduction
  if ((threadIdx.x & 63) == 0) smem[wave] = v;
  __syncthreads();
  float r = smem[0];
  for (int w = 1; w < nwaves; ++w)
    r = OP == Red::kMin ? fminf(r, smem[w]) : OP == Red::kMax ? fmaxf(r, smem[w]) : r + smem[w];
  return r;
}

// ---- pass 1: min over finite pixels + count of non-finite ones ----------------
// (slots != nullptr: the workgroup's results go to the statistic slots instead of partial[])
__global__ __launch_bounds__(256) void lk_stats1(const float *__restrict__ img, size_t npx,
                                                 float *__restrict__ partial, unsigned *__restrict__ slots) {
  float mn = INFINITY, bad = 0.f;
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  const size_t first = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  auto take = [&](float v) {
    const bool fin = isfinite(v);
    mn = fminf(mn, fin ? v : INFINITY);
    bad += fin ? 0.f : 1.f;
  };
  // 16-byte loads, four in flight per thread (a streaming read is bound by bytes in flight)
  const size_t n4 = (reinterpret_cast<uintptr_t>(img) % 16 == 0) ? npx / 4 : 0;
  const float4 *img4 = reinterpret_cast<const float4 *>(img);
  size_t i = first;
  for (; i + 3 * stride < n4; i += 4 * stride) {
    const float4 a = img4[i], b = img4[i + stride], c = img4[i + 2 * stride], d = img4[i + 3 * stride];
    take(a.x), take(a.y), take(a.z), take(a.w);
    take(b.x), take(b.y), take(b.z), take(b.w);
    take(c.x), take(c.y), take(c.z), take(c.w);
    take(d.x), take(d.y), take(d.z), take(d.w);
  }
  for (; i < n4; i += stride) {
    const float4 a = img4[i];
    take(a.x), take(a.y), take(a.z), take(a.w);
  }
  for (size_t j = 4 * n4 + first; j < npx; j += stride) take(img[j]);
  __shared__ float s[2][4];
  mn = wave_min(mn);
  bad = wave_sum(bad);
  if ((threadIdx.x & 63) == 0) {
    s[0][threadIdx.x >> 6] = mn;
    s[1][threadIdx.x >> 6] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float b_min = fminf(fminf(s[0][0], s[0][1]), fminf(s[0][2], s[0][3]));
    const float b_bad = s[1][0] + s[1][1] + s[1][2] + s[1][3];
    if (slots) {
      slot_min(slots, kSlMin, blockIdx.x, b_min);
      if (b_bad > 0.f) atomicAdd(&slots[kSlNan * kSlots + (blockIdx.x & (kSlots - 1))], static_cast<unsigned>(b_bad));
    } else {
      partial[blockIdx.x] = b_min;
      partial[gridDim.x + blockIdx.x] = b_bad;
    }
  }
}

__global__ __launch_bounds__(kFinalThreads) void lk_stats1_final(const float *__restrict__ partial,
                                                                 int nb,
                                                                 float *__restrict__ stats) {
  __shared__ float smem[16];
  float mn = INFINITY, bad = 0.f;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) {
    mn = fminf(mn, partial[i]);
    bad += partial[nb + i];
  }
  mn = block_reduce<Red::kMin>(mn, smem);
  bad = block_reduce<Red::kSum>(bad, smem);
  if (threadIdx.x == 0) {
    stats[kMinAll] = mn;
    stats[kNanCount] = bad;
  }
}

// ---- pass 2: binary opening (3x3 cross) + statistics of the cleaned frame ------
// field = (filled > min).  Opening = erode then dilate with the plus-shaped 3x3
// element, image border neutral.  Pixels of the field that the opening removes
// are set to the minimum (images.py:78-81).
// The morphology is done on BIT MASKS (rounds 1-2 staged tiles in LDS and spent the pass in
// byte-sized LDS reads, 11 per pixel): a wave owns 64 image columns (the outer two on each side are
// halo, 60 are written) and 32 output rows.  It loads its 36 rows first (all loads in flight together)
// and turns every row into two 64-bit masks with one compare each - FIN: finite, F: above the minimum.
// Rounds 3-4 then walked the rows with the masks in SCALAR registers: 1090 scalar instructions per wave,
// the scalar pipe 62 % busy, 48 us at 4096^2 (profiles/r04/g_prep_pmc.csv).  Here the masks are
// TRANSPOSED: row q's masks are moved into lane q, and the 3x3 cross becomes a handful of 64-bit
// VALU operations for all rows at once - columns by shifts inside the word, rows by DPP moves between lanes:
//    A = F | N (N: outside the image, neutral for the erosion);
//    E_y = F_y & (A_y << 1) & (A_y >> 1) & A_{y-1} & A_{y+1};
//    O_y = E_y | (E_y << 1) | (E_y >> 1) | E_{y-1} | E_{y+1};   removed = F & ~O;   keep = FIN & ~removed
// Lane o ends up with the words of OUTPUT row o.  The keep words go to memory straight from the lanes; for
// the statistics one mask per row (kept pixels of the written columns) comes back to scalar registers by
// v_readlane and selects the values that count: a removed pixel becomes the minimum, which is below every
// finite value, so max / min over the cleaned row = max / min over the kept values, folded with the minimum
// if the row lost a pixel (a per-row flag from the transposed side).
constexpr int kOpenRowsW = 16;        // float64 twin: output rows per wave
constexpr int kOpenColsW = 60;        // output columns per wave (64 lanes - 2 x 2 halo)
constexpr int kOpenRowsWG = 4 * kOpenRowsW;
constexpr int kOpenRows32 = 32;       // this kernel: output rows per wave
constexpr int kOpenRowsWG32 = 4 * kOpenRows32;

__device__ __forceinline__ unsigned long long next_lane_u64(unsigned long long v) {  // lane i gets lane i + 1's word
  const unsigned lo = static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x130, 0xf, 0xf, true));
  const unsigned hi = static_cast<unsigned>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v >> 32), 0x130, 0xf, 0xf, true));
  return (static_cast<unsigned long long>(hi) << 32) | lo;
}

// slots != nullptr: minimum and NaN count are read from the statistic slots (lk_stats1 wrote them), the
// results go there too, and workgroup (0, 0) writes the two input statistics into stats[] for later readers.
// clean == nullptr: the cleaned frame is not stored, keepbits gets one word per (row, strip) instead
__global__ __launch_bounds__(256) void lk_open_bits(const float *__restrict__ img, int m, int n,
                                                    int size_opening, int buffer_mask,
                                                    float *__restrict__ stats,
                                                    float *__restrict__ clean,
                                                    float *__restrict__ partial, Band band,
                                                    unsigned *__restrict__ slots,
                                                    unsigned long long *__restrict__ keepbits) {
  __shared__ float red[3][4];
  const float mn = slots ? slots_min(slots, kSlMin) : stats[kMinAll];
  const float nan_count = slots ? slots_count(slots, kSlNan) : stats[kNanCount];
  if (slots && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
    stats[kMinAll] = mn;
    stats[kNanCount] = nan_count;
  }
  // (readfirstlane: the wave index is the same in every lane - row arithmetic stays scalar)
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int x = blockIdx.x * kOpenColsW - 2 + lane;
  const int yb = blockIdx.y * kOpenRowsWG32 + wave * kOpenRows32;  // first output row of the wave
  const bool col_in = x >= 0 && x < n;
  constexpr int kLoad = kOpenRows32 + 4;
  float mx_all = -INFINITY, mn_feat = INFINITY, mx_feat = -INFINITY;
  if (yb < m) {  // (uniform)
    // every load is inside the image (clamped row and column): what lies outside is masked on the
    // transposed side, no load waits for a branch
    const float *colp = img + min(max(x, 0), n - 1);
    float v[kLoad];
#pragma unroll
    for (int q = 0; q < kLoad; ++q) v[q] = colp[static_cast<size_t>(min(max(yb - 2 + q, 0), m - 1)) * n];
    unsigned f_lo = 0, f_hi = 0, fin_lo = 0, fin_hi = 0;  // lane q: masks of loaded row q
#pragma unroll
    for (int q = 0; q < kLoad; ++q) {
      const unsigned long long fin = __ballot(isfinite(v[q]));
      const unsigned long long f = __ballot(v[q] > mn);
      const bool mine = lane == q;  // (what v_writelane_b32 does; no builtin for it in this compiler)
      fin_lo = mine ? static_cast<unsigned>(fin) : fin_lo;
      fin_hi = mine ? static_cast<unsigned>(fin >> 32) : fin_hi;
      f_lo = mine ? static_cast<unsigned>(f) : f_lo;
      f_hi = mine ? static_cast<unsigned>(f >> 32) : f_hi;
    }
    // ---- transposed side: lane q works on loaded row q = image row yb - 2 + q ----
    const unsigned long long colmask = __ballot(col_in);
    const unsigned long long wmask = __ballot(lane >= 2 && lane < 2 + kOpenColsW && col_in);  // written columns
    const int yq = yb - 2 + lane;
    const bool row_in = lane < kLoad && yq >= 0 && yq < m;
    const unsigned long long FIN = row_in ? (((static_cast<unsigned long long>(fin_hi) << 32) | fin_lo) & colmask) : 0ull;
    const unsigned long long F = ((static_cast<unsigned long long>(f_hi) << 32) | f_lo) & FIN;  // masked pixels are filled with the minimum
    const unsigned long long A = row_in ? (F | ~colmask) : ~0ull;  // outside the image: neutral for the erosion
    const unsigned long long HE = F & (A << 1) & (A >> 1);
    const unsigned long long E1 = next_lane_u64(HE) & A & next_lane_u64(next_lane_u64(A));  // erosion of row q + 1
    const unsigned long long HO1 = E1 | (E1 << 1) | (E1 >> 1);
    const unsigned long long O2 = next_lane_u64(HO1) | E1 | next_lane_u64(next_lane_u64(E1));  // opening of row q + 2
    const unsigned long long F2 = next_lane_u64(next_lane_u64(F)), FIN2 = next_lane_u64(next_lane_u64(FIN));
    // lane o now holds OUTPUT row o = image row yb + o
    const int y = yb + lane;
    const bool out_row = lane < kOpenRows32 && y < m;
    const unsigned long long removed = size_opening > 0 ? (F2 & ~O2) : 0ull;  // field pixels the opening takes away
    const unsigned long long keep = FIN2 & ~removed;
    if (!clean && out_row) {
      // one word per (row, strip): which pixels KEEP their value (finite and not removed; every other pixel
      // of the cleaned frame is the minimum) - lk_to_u8_bits reads the frame itself beside these words;
      // bit = lane of the column (2 .. 61 are the strip's pixels)
      keepbits[static_cast<size_t>(y) * gridDim.x + blockIdx.x] = keep;
    }
    // shitomasi.py:140 masks row 0 always and row 1 when anything is masked
    const int first_row = buffer_mask > 0 ? (nan_count > 0.f ? 2 : 1) : 0;
    const bool counted_row = out_row && y >= band.lo && y < band.hi;
    const unsigned long long kept_counted = counted_row ? (keep & wmask) : 0ull;  // their values count as they are
    const unsigned k_lo = static_cast<unsigned>(kept_counted), k_hi = static_cast<unsigned>(kept_counted >> 32);
    const unsigned r_lo = static_cast<unsigned>(removed), r_hi = static_cast<unsigned>(removed >> 32);
    // rows that lost a counted pixel: the minimum is among their values
    const unsigned long long lost_rows = __ballot(counted_row && (removed & wmask) != 0ull);
    // rows 0 and 1 of the wave may lie above first_row: their statistics are kept apart
    float mx0 = -INFINITY, mn0 = INFINITY, mx1 = -INFINITY, mn1 = INFINITY, mxr = -INFINITY, mnr = INFINITY;
    const bool writer = lane >= 2 && lane < 2 + kOpenColsW && col_in;
#pragma unroll
    for (int o = 0; o < kOpenRows32; ++o) {
      const unsigned long long K = (static_cast<unsigned long long>(__builtin_amdgcn_readlane(k_hi, o)) << 32) |
                                   static_cast<unsigned>(__builtin_amdgcn_readlane(k_lo, o));
      const bool kept = __builtin_amdgcn_inverse_ballot_w64(K);
      const float hi = kept ? v[o + 2] : -INFINITY, lo = kept ? v[o + 2] : INFINITY;
      if (o == 0) {
        mx0 = max_plain(mx0, hi), mn0 = min_plain(mn0, lo);
      } else if (o == 1) {
        mx1 = max_plain(mx1, hi), mn1 = min_plain(mn1, lo);
      } else {
        mxr = max_plain(mxr, hi), mnr = min_plain(mnr, lo);
      }
      if (clean) {  // (uniform) the entry points that return the cleaned frame
        const unsigned long long R = (static_cast<unsigned long long>(__builtin_amdgcn_readlane(r_hi, o)) << 32) |
                                     static_cast<unsigned>(__builtin_amdgcn_readlane(r_lo, o));
        const float val = __builtin_amdgcn_inverse_ballot_w64(R) ? mn : v[o + 2];
        if (writer && yb + o < m) clean[static_cast<size_t>(yb + o) * n + x] = val;
      }
    }
    const bool feat0 = yb + band.y_org >= first_row, feat1 = yb + 1 + band.y_org >= first_row;  // (uniform)
    mx_all = max_plain(max_plain(mx0, mx1), mxr);
    mx_feat = max_plain(max_plain(feat0 ? mx0 : -INFINITY, feat1 ? mx1 : -INFINITY), mxr);
    mn_feat = min_plain(min_plain(feat0 ? mn0 : INFINITY, feat1 ? mn1 : INFINITY), mnr);
    if (lost_rows != 0ull) mx_all = max_plain(mx_all, mn);
    if ((lost_rows & ~((feat0 ? 0ull : 1ull) | (feat1 ? 0ull : 2ull))) != 0ull) {
      mx_feat = max_plain(mx_feat, mn);
      mn_feat = min_plain(mn_feat, mn);
    }
  }
  mx_all = wave_max(mx_all);
  mn_feat = wave_min(mn_feat);
  mx_feat = wave_max(mx_feat);
  if (lane == 0) {
    red[0][wave] = mx_all;
    red[1][wave] = mn_feat;
    red[2][wave] = mx_feat;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int b = blockIdx.y * gridDim.x + blockIdx.x, nb = gridDim.x * gridDim.y;
    const float b_max = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
    const float b_fmin = fminf(fminf(red[1][0], red[1][1]), fminf(red[1][2], red[1][3]));
    const float b_fmax = fmaxf(fmaxf(red[2][0], red[2][1]), fmaxf(red[2][2], red[2][3]));
    if (slots) {
      slot_max(slots, kSlMaxAll, b, b_max);
      slot_min(slots, kSlMinFeat, b, b_fmin);
      slot_max(slots, kSlMaxFeat, b, b_fmax);
    } else {
      partial[b] = b_max;
      partial[nb + b] = b_fmin;
      partial[2 * nb + b] = b_fmax;
    }
  }
}

__global__ __launch_bounds__(kFinalThreads) void lk_open_final(const float *__restrict__ partial,
                                                               int nb, float *__restrict__ stats) {
  __shared__ float smem[16];
  float a = -INFINITY, b = INFINITY, c = -INFINITY;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) {
    a = fmaxf(a, partial[i]);
    b = fminf(b, partial[nb + i]);
    c = fmaxf(c, partial[2 * nb + i]);
  }
  a = block_reduce<Red::kMax>(a, smem);
  b = block_reduce<Red::kMin>(b, smem);
  c = block_reduce<Red::kMax>(c, smem);
  if (threadIdx.x == 0) {
    stats[kMaxAll] = a;
    stats[kMinFeat] = b;
    stats[kMaxFeat] = c;
  }
}

// ---- pass 3: min-max rescale to uint8 by truncation ----------------------------
// tracking/lucaskanade.py:143-160 (all finite pixels) and shitomasi.py:143-151
// (rows hidden by the :140 quirk are filled with the minimum first).
__device__ __forceinline__ unsigned char quantise(float v, float lo, float hi) {
  float s = (hi - lo) > 1e-8f ? (v - lo) / (hi - lo) * 255.f : v - lo;
  // astype(uint8) truncates toward zero; out-of-range values cannot occur for lo <= v <= hi
  return static_cast<unsigned char>(static_cast<int>(s));
}

// slots != nullptr: the three statistics of the cleaned frame are read from the statistic slots
// (lk_open_bits wrote them) and workgroup 0 writes them into stats[] for later readers
__global__ __launch_bounds__(256) void lk_to_u8(const float *__restrict__ clean, int m, int n,
                                                int buffer_mask, float *__restrict__ stats,
                                                unsigned char *__restrict__ trk,
                                                unsigned char *__restrict__ feat, int y_org,
                                                const unsigned *__restrict__ slots) {
  const float fill = stats[kMinAll], hi = slots ? slots_max(slots, kSlMaxAll) : stats[kMaxAll];
  const float flo = slots ? slots_min(slots, kSlMinFeat) : stats[kMinFeat];
  const float fhi = slots ? slots_max(slots, kSlMaxFeat) : stats[kMaxFeat];
  if (slots && blockIdx.x == 0 && threadIdx.x == 0) {
    stats[kMaxAll] = hi;
    stats[kMinFeat] = flo;
    stats[kMaxFeat] = fhi;
  }
  const int first_row = max((buffer_mask > 0 ? (stats[kNanCount] > 0.f ? 2 : 1) : 0) - y_org, 0);
  const size_t npx = static_cast<size_t>(m) * n;
  const size_t first_feature_px = static_cast<size_t>(first_row) * n;
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x * 4;
  for (size_t i = (static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x) * 4; i < npx;
       i += stride) {
    unsigned char t[4], f[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const size_t p = i + j;
      float v = p < npx ? clean[p] : fill;
      const bool ok = isfinite(v);
      if (!ok) v = fill;
      t[j] = quantise(v, fill, hi);
      f[j] = quantise((ok && p >= first_feature_px) ? v : fill, flo, fhi);  // rows >= first_row
    }
    if (i + 3 < npx && (npx & 3) == 0) {
      *reinterpret_cast<uchar4 *>(trk + i) = make_uchar4(t[0], t[1], t[2], t[3]);
      if (feat) *reinterpret_cast<uchar4 *>(feat + i) = make_uchar4(f[0], f[1], f[2], f[3]);
    } else {
      for (int j = 0; j < 4 && i + j < npx; ++j) {
        trk[i + j] = t[j];
        if (feat) feat[i + j] = f[j];
      }
    }
  }
}

// The same rendering from the FRAME and the keep bits of lk_open_bits (the resident estimate: the cleaned
// frame is never stored - 8 of the 18 bytes per pixel the three passes moved).  A thread renders four
// adjacent pixels of kU8Rows rows; all its loads are issued before the first value is used.  VEC: rows
// are 16-byte aligned (n % 4 == 0, aligned pointers).
constexpr int kU8Rows = 4;
template <bool VEC>
__global__ __launch_bounds__(256) void lk_to_u8_bits(const float *__restrict__ img,
                                                     const unsigned long long *__restrict__ keepbits, int nstrips,
                                                     int m, int n, int buffer_mask, float *__restrict__ stats,
                                                     unsigned char *__restrict__ trk, unsigned char *__restrict__ feat,
                                                     const unsigned *__restrict__ slots) {
  const float fill = stats[kMinAll], hi = slots_max(slots, kSlMaxAll);
  const float flo = slots_min(slots, kSlMinFeat), fhi = slots_max(slots, kSlMaxFeat);
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
    stats[kMaxAll] = hi;
    stats[kMinFeat] = flo;
    stats[kMaxFeat] = fhi;
  }
  const int first_row = buffer_mask > 0 ? (stats[kNanCount] > 0.f ? 2 : 1) : 0;
  // the two renderings differ only when the hidden rows hold an extreme of the frame: as a rule one
  // division per pixel instead of two (uniform)
  const bool same_scale = flo == fill && fhi == hi;
  const int x = (blockIdx.x * 256 + threadIdx.x) * 4;
  const int y0 = blockIdx.y * kU8Rows;
  if (x >= n) return;
  const int strip = x / kOpenColsW, shift = x - strip * kOpenColsW + 2;  // (60 % 4 == 0: the four pixels share a word)
  float v[kU8Rows][4];
  unsigned long long w[kU8Rows];
#pragma unroll
  for (int r = 0; r < kU8Rows; ++r) {
    const int y = min(y0 + r, m - 1);
    const float *row = img + static_cast<size_t>(y) * n + x;
    w[r] = keepbits[static_cast<size_t>(y) * nstrips + strip];
    if (VEC) {
      const float4 q = *reinterpret_cast<const float4 *>(row);
      v[r][0] = q.x, v[r][1] = q.y, v[r][2] = q.z, v[r][3] = q.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[r][j] = x + j < n ? row[j] : 0.f;
    }
  }
#pragma unroll
  for (int r = 0; r < kU8Rows; ++r) {
    const int y = y0 + r;
    if (y >= m) break;
    const unsigned keep = static_cast<unsigned>(w[r] >> shift);
    unsigned t = 0, f = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool k = (keep >> j) & 1u;
      const float val = k ? v[r][j] : fill;
      t |= static_cast<unsigned>(quantise(val, fill, hi)) << (8 * j);
      if (!same_scale) f |= static_cast<unsigned>(quantise(y >= first_row ? val : fill, flo, fhi)) << (8 * j);
    }
    // (same bounds: the feature rendering IS the tracking rendering, hidden rows are the minimum = 0)
    if (same_scale) f = y >= first_row ? t : 0u;
    const size_t at = static_cast<size_t>(y) * n + x;
    if (VEC) {
      *reinterpret_cast<unsigned *>(trk + at) = t;
      if (feat) *reinterpret_cast<unsigned *>(feat + at) = f;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (x + j >= n) break;
        trk[at + j] = static_cast<unsigned char>(t >> (8 * j));
        if (feat) feat[at + j] = static_cast<unsigned char>(f >> (8 * j));
      }
    }
  }
}

// ---- float64 frames: the three frame passes in double ---------------------------------------
// The reference cleans and quantises a frame in the dtype it is given (pysteps arrays are float64
// as a rule): the minimum, the `> minimum` test of the opening, the min-max rescale and its
// truncation to uint8 all happen in double there (utils/images.py:58-86,
// tracking/lucaskanade.py:135-160, feature/shitomasi.py:128-151).  Rounding the frame to float32
// first moves a pixel across a grey-level boundary now and then (~2e-5 of the pixels), so float64
// frames get double-precision twins of the three passes; everything downstream works on the uint8
// renderings and on the float32 copy of the cleaned frame (used for its NaN pattern only).
// dstats: [0] min over finite pixels, [1] max after opening, [2] / [3] min / max of the feature rows.
__device__ __forceinline__ double wave_min_d(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = fmin(v, __shfl_xor(v, d));
  return v;
}
__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = fmax(v, __shfl_xor(v, d));
  return v;
}

__global__ __launch_bounds__(256) void lk_stats1_f64(const double *__restrict__ img, size_t npx,
                                                     double *__restrict__ partial) {
  double mn = INFINITY, bad = 0.0;
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < npx; i += stride) {
    const double v = img[i];
    const bool fin = isfinite(v);
    mn = fmin(mn, fin ? v : INFINITY);
    bad += fin ? 0.0 : 1.0;
  }
  __shared__ double s[2][4];
  mn = wave_min_d(mn);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) bad += __shfl_xor(bad, d);
  if ((threadIdx.x & 63) == 0) {
    s[0][threadIdx.x >> 6] = mn;
    s[1][threadIdx.x >> 6] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = fmin(fmin(s[0][0], s[0][1]), fmin(s[0][2], s[0][3]));
    partial[gridDim.x + blockIdx.x] = s[1][0] + s[1][1] + s[1][2] + s[1][3];
  }
}

// one block: finishes either reduction (what = 0: stats pass, 1: opening pass)
__global__ __launch_bounds__(kFinalThreads) void lk_final_f64(const double *__restrict__ partial, int nb, int what,
                                                             float *__restrict__ stats, double *__restrict__ dstats) {
  __shared__ double sm[3][16];
  double a = what == 0 ? INFINITY : -INFINITY, b = what == 0 ? 0.0 : INFINITY, c = -INFINITY;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) {
    if (what == 0) {
      a = fmin(a, partial[i]);
      b += partial[nb + i];
    } else {
      a = fmax(a, partial[i]);
      b = fmin(b, partial[nb + i]);
      c = fmax(c, partial[2 * nb + i]);
    }
  }
  if (what == 0) {
    a = wave_min_d(a);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) b += __shfl_xor(b, d);
  } else {
    a = wave_max_d(a);
    b = wave_min_d(b);
    c = wave_max_d(c);
  }
  const int wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sm[0][wave] = a;
    sm[1][wave] = b;
    sm[2][wave] = c;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < nwaves; ++w) {
      if (what == 0) {
        a = fmin(a, sm[0][w]);
        b += sm[1][w];
      } else {
        a = fmax(a, sm[0][w]);
        b = fmin(b, sm[1][w]);
        c = fmax(c, sm[2][w]);
      }
    }
    if (what == 0) {
      dstats[0] = a;
      stats[kMinAll] = static_cast<float>(a);
      stats[kNanCount] = static_cast<float>(b);
    } else {
      dstats[1] = a;
      dstats[2] = b;
      dstats[3] = c;
      stats[kMaxAll] = static_cast<float>(a);
      stats[kMinFeat] = static_cast<float>(b);
      stats[kMaxFeat] = static_cast<float>(c);
    }
  }
}

// lk_open_bits for a float64 frame: clean64 = the cleaned frame in double (for the rescale),
// clean32 = its float32 copy (NaN pattern for the later passes)
__global__ __launch_bounds__(256) void lk_open_bits_f64(const double *__restrict__ img, int m, int n,
                                                        int size_opening, int buffer_mask,
                                                        const float *__restrict__ stats,
                                                        const double *__restrict__ dstats,
                                                        float *__restrict__ clean32, double *__restrict__ clean64,
                                                        double *__restrict__ partial) {
  __shared__ double red[3][4];
  const double mn = dstats[0];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x = blockIdx.x * kOpenColsW - 2 + lane;
  const int yb = blockIdx.y * kOpenRowsWG + wave * kOpenRowsW;
  const bool col_in = x >= 0 && x < n;
  constexpr int kLoad = kOpenRowsW + 4;
  double v[kLoad];
#pragma unroll
  for (int q = 0; q < kLoad; ++q) {
    const int y = yb - 2 + q;
    v[q] = (col_in && y >= 0 && y < m) ? img[static_cast<size_t>(y) * n + x] : 0.0;
  }
  unsigned long long A[kLoad], F[kLoad];
#pragma unroll
  for (int q = 0; q < kLoad; ++q) {
    const int y = yb - 2 + q;
    const bool row_in = y >= 0 && y < m;
    F[q] = __ballot(row_in && col_in && isfinite(v[q]) && v[q] > mn);
    A[q] = F[q] | __ballot(!(row_in && col_in));
  }
  unsigned long long E[kLoad];
#pragma unroll
  for (int q = 1; q < kLoad - 1; ++q) E[q] = F[q] & (A[q] << 1) & (A[q] >> 1) & A[q - 1] & A[q + 1];
  double mx_all = -INFINITY, mn_feat = INFINITY, mx_feat = -INFINITY;
  const int first_row = buffer_mask > 0 ? (stats[kNanCount] > 0.f ? 2 : 1) : 0;
  const bool writer = lane >= 2 && lane < 2 + kOpenColsW && col_in;
#pragma unroll
  for (int q = 2; q < kLoad - 2; ++q) {
    const int y = yb - 2 + q;
    if (y >= m) break;  // (uniform)
    const unsigned long long O = E[q] | (E[q] << 1) | (E[q] >> 1) | E[q - 1] | E[q + 1];
    double val = v[q];
    if (size_opening > 0 && ((F[q] >> lane) & 1ull) && !((O >> lane) & 1ull)) val = mn;
    if (writer) {
      if (isfinite(val)) {
        mx_all = fmax(mx_all, val);
        if (y >= first_row) {
          mn_feat = fmin(mn_feat, val);
          mx_feat = fmax(mx_feat, val);
        }
      }
      clean64[static_cast<size_t>(y) * n + x] = val;
      clean32[static_cast<size_t>(y) * n + x] = static_cast<float>(val);
    }
  }
  mx_all = wave_max_d(mx_all);
  mn_feat = wave_min_d(mn_feat);
  mx_feat = wave_max_d(mx_feat);
  if (lane == 0) {
    red[0][wave] = mx_all;
    red[1][wave] = mn_feat;
    red[2][wave] = mx_feat;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int b = blockIdx.y * gridDim.x + blockIdx.x, nb = gridDim.x * gridDim.y;
    partial[b] = fmax(fmax(red[0][0], red[0][1]), fmax(red[0][2], red[0][3]));
    partial[nb + b] = fmin(fmin(red[1][0], red[1][1]), fmin(red[1][2], red[1][3]));
    partial[2 * nb + b] = fmax(fmax(red[2][0], red[2][1]), fmax(red[2][2], red[2][3]));
  }
}

__device__ __forceinline__ unsigned char quantise_f64(double v, double lo, double hi) {
  const double s = (hi - lo) > 1e-8 ? (v - lo) / (hi - lo) * 255.0 : v - lo;
  return static_cast<unsigned char>(static_cast<int>(s));  // astype(uint8) truncates toward zero
}

__global__ __launch_bounds__(256) void lk_to_u8_f64(const double *__restrict__ clean, int m, int n, int buffer_mask,
                                                    const float *__restrict__ stats,
                                                    const double *__restrict__ dstats,
                                                    unsigned char *__restrict__ trk, unsigned char *__restrict__ feat) {
  const double fill = dstats[0], hi = dstats[1], flo = dstats[2], fhi = dstats[3];
  const int first_row = buffer_mask > 0 ? (stats[kNanCount] > 0.f ? 2 : 1) : 0;
  const size_t npx = static_cast<size_t>(m) * n;
  const size_t first_feature_px = static_cast<size_t>(first_row) * n;
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t p = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; p < npx; p += stride) {
    double v = clean[p];
    const bool ok = isfinite(v);
    if (!ok) v = fill;
    trk[p] = quantise_f64(v, fill, hi);
    if (feat) feat[p] = quantise_f64((ok && p >= first_feature_px) ? v : fill, flo, fhi);
  }
}

// ---- Shi-Tomasi response: cv::cornerMinEigenVal(8U, blockSize, ksize=3) --------
constexpr int kMaxBlockR = 3;  // block_size <= 7

__device__ __forceinline__ bool px_allowed(const float *__restrict__ clean, int m, int n, int x,
                                           int y, int bm, bool any_nan) {
  // allowed = NOT dilate(nan_mask, ones(bm,bm)) (shitomasi.py:135-139,152)
  if (!any_nan) return true;
  if (bm <= 0) return isfinite(clean[static_cast<size_t>(y) * n + x]);
  const int a = bm / 2;
  for (int j = 0; j < bm; ++j) {
    const int yy = y + j - a;
    if (yy < 0 || yy >= m) continue;
    for (int i = 0; i < bm; ++i) {
      const int xx = x + i - a;
      if (xx < 0 || xx >= n) continue;
      if (!isfinite(clean[static_cast<size_t>(yy) * n + xx])) return false;
    }
  }
  return true;
}

// Per pixel (OpenCV cornerMinEigenVal, restated in oracle/lk_opencv.py): Sobel derivatives of the
// 3x3 neighbourhood a[row][col] with the scale s = 1 / (4 block_size 255) folded in,
//     dx = ((a02 - a00) + (a22 - a20)) s + (a12 - a10) 2s
//     dy = ((a20 + a22) s + a21 2s) - ((a00 + a02) s + a01 2s)
// (float32, every product and sum rounded: the expression tree below keeps exactly these roundings),
// the products dx dx, dx dy, dy dy summed over the block_size x block_size window (boxFilter: float
// products accumulated in double, BORDER_REFLECT_101 on the product images), lambda_min of the sums.
//
// Column-walking form: nothing goes through LDS, a lane owns one image COLUMN, a wave walks
// ROWS + 2 (r + 1) rows of a 64-column strip from top to bottom and keeps everything in registers.
// (Rounds 1-3 staged a 32 x 32 tile and three product arrays in LDS and spent the pass waiting for
// them - bank conflicts of the double-precision strips, two barriers, 0.29 of the VALU issue slots
// busy: 106 us at 4096^2; this form 63 us alone, 77 us beside the next frame's passes.)
//  * per loaded row (one byte per lane; the neighbours' bytes come from the next lanes by DPP, so a
//    lane works for the column one to the right of the one it loads): the horizontal difference
//    Hd = right - left and the smoothed value G = (left + right) s + centre 2s - exact small integers
//    until the multiplications;
//  * per row: dx = (Hd[-1] + Hd[+1]) s + Hd[0] 2s, dy = G[+1] - G[-1], the three products, and the
//    vertical box sums as SLIDING column sums in double: V += P(new) - P(row leaving the window).
//    The products span 20 binary orders of magnitude with 24-bit mantissas, so every partial sum of a
//    7 x 7 window is EXACT in double: adding and subtracting in any order gives the bits of
//    boxFilter's accumulation; the last BS product rows wait in a register ring;
//  * the horizontal box sum takes V from the next 2r lanes (64-bit DPP moves), then the eigenvalue.
// Image borders: the pixel loads are reflected (reflect-101 rows and columns); a product OUTSIDE the
// image has to be the product at its mirror position (boxFilter's border), and the walked stencil
// there is the mirror image of the true one: its dx (columns) or dy (rows) comes out with the
// opposite sign - exactly, negation commutes with every rounding -, so the sign of s is flipped per
// lane and the sign of dy per row where the position is mirrored.
// 4 waves = 4 row bands per workgroup; lanes 0 .. 63 - 2 (r + 1) write.
__device__ __forceinline__ float next_lane_f(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x130 /* wave_shl:1 */, 0xf, 0xf, true));
}
__device__ __forceinline__ double next_lane_d(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x130, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x130, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
// true where a stencil walked through reflected coordinates comes out mirrored (i + 1 maps to the
// pixel BEFORE the image of i); turning points have equal neighbours on both sides: either answer
__device__ __forceinline__ bool walk_mirrored(int i, int n) {
  if (i >= 0 && i + 1 < n) return false;
  return reflect101(i + 1, n) != reflect101(reflect101(i, n) + 1, n);
}

constexpr int crn_cols(int block_size) { return 64 - 2 * (block_size / 2 + 1); }  // output columns per wave

template <int BS, int ROWS>
__global__ __launch_bounds__(256) void lk_corner_response_cols(
    const unsigned char *__restrict__ u8, const float *__restrict__ clean, int m, int n,
    int buffer_mask, const float *__restrict__ stats, float *__restrict__ eig,
    float *__restrict__ partial, Band band, unsigned *__restrict__ slots, int *__restrict__ zero_a, int count_a,
    int *__restrict__ zero_b, int count_b) {
  constexpr int r = BS / 2, H = r + 1, W = crn_cols(BS);
  // (zero_a / zero_b: counters and scratch the NEXT kernels expect cleared - done by the first workgroup
  // here instead of one 5 us fill launch each)
  if (blockIdx.x == 0 && blockIdx.y == 0) {
    for (int i = threadIdx.x; i < count_a; i += 256) zero_a[i] = 0;
    for (int i = threadIdx.x; i < count_b; i += 256) zero_b[i] = 0;
  }
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int x0 = blockIdx.x * W;
  const int yb = (blockIdx.y * 4 + wave) * ROWS;  // first output row of the wave
  float best = 0.f;
  if (yb < m) {
    const float s = 1.0f / (4.0f * static_cast<float>(BS) * 255.0f), s2 = 2.f * s;
    const int xl = x0 - H + lane;  // column this lane loads; its products belong to column xl + 1
    const bool neg_x = walk_mirrored(xl + 1, n);
    const float sx = neg_x ? -s : s, sx2 = neg_x ? -s2 : s2;
    const unsigned char *col = u8 + reflect101(xl, n);
    // rows are reflected at most once unless the image is only a few rows high (scalar arithmetic per
    // row: keep the division of the general form out of the walk).  The walk itself reaches row m + r; the preload
    // below runs up to BS rows ahead of the last product row, as far as row m + 3 BS - r - 2, and a single reflection
    // of that row, 2 m - 2 - y, has to stay in the image as well: m >= 3 BS - r
    constexpr int kFewRows = 2 * H + 2 > 3 * BS - r ? 2 * H + 2 : 3 * BS - r;
    const bool few_rows = m < kFewRows;
    auto row_of = [&](int y) -> int {
      if (few_rows) return reflect101(y, m);
      y = y < 0 ? -y : y;
      return y >= m ? 2 * m - 2 - y : y;
    };
    // sequence row i is image row yb - H + i
    auto load_row = [&](int i) -> int { return col[static_cast<size_t>(row_of(yb - H + i)) * n]; };
    auto row_terms = [&](int raw, float &hd, float &g) {
      const float a = static_cast<float>(raw);  // left
      const float c = next_lane_f(a);           // centre
      const float b = next_lane_f(c);           // right
      hd = b - a;
      g = (a + b) * s + c * s2;
    };
    const bool any_nan = stats[kNanCount] > 0.f;
    const int x = x0 + lane;  // output column of the lane
    const bool writer = lane < W && x < n;
    const int rows_out = min(ROWS, m - yb);
    const int last_p = rows_out + BS - 1;  // product rows 1 .. last_p; output row o = p - BS
    double ring[3][BS], V[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < BS; ++j) ring[0][j] = ring[1][j] = ring[2][j] = 0.0;
    int raw[BS];
    const int raw0 = load_row(0), raw1 = load_row(1);
#pragma unroll
    for (int j = 0; j < BS; ++j) raw[j] = load_row(2 + j);
    float hd_m, hd_0, g_m, g_0;
    row_terms(raw0, hd_m, g_m);
    row_terms(raw1, hd_0, g_0);
    for (int base = 1; base <= last_p; base += BS) {
      int nxt[BS];
#pragma unroll
      for (int j = 0; j < BS; ++j) nxt[j] = load_row(base + BS + 1 + j);  // (inside the image: see kFewRows)
#pragma unroll
      for (int j = 0; j < BS; ++j) {
        const int p = base + j;
        if (p > last_p) break;  // (uniform)
        constexpr int kRingBase = 1;
        const int slot = (kRingBase + j) % BS;  // = p % BS, a constant after unrolling
        float hd_p, g_p;
        row_terms(raw[j], hd_p, g_p);  // sequence row p + 1
        const float dx = (hd_m + hd_p) * sx + hd_0 * sx2;
        float dy = g_p - g_m;
        const int y_seq = yb - H + p;
        const bool row_mirrored = few_rows ? walk_mirrored(y_seq, m) : (y_seq < 0 || y_seq >= m);
        const unsigned row_sign = row_mirrored ? 0x80000000u : 0u;  // (scalar)
        dy = __uint_as_float(__float_as_uint(dy) ^ row_sign);
        const double pxx = static_cast<double>(dx * dx), pxy = static_cast<double>(dx * dy);
        const double pyy = static_cast<double>(dy * dy);
        V[0] += pxx - ring[0][slot];
        V[1] += pxy - ring[1][slot];
        V[2] += pyy - ring[2][slot];
        ring[0][slot] = pxx;
        ring[1][slot] = pxy;
        ring[2][slot] = pyy;
        hd_m = hd_0;
        hd_0 = hd_p;
        g_m = g_0;
        g_0 = g_p;
        if (p >= BS) {
          double w0 = V[0], w1 = V[1], w2 = V[2];
          double t0 = V[0], t1 = V[1], t2 = V[2];
#pragma unroll
          for (int c = 0; c < 2 * r; ++c) {
            t0 = next_lane_d(t0);
            t1 = next_lane_d(t1);
            t2 = next_lane_d(t2);
            w0 += t0;
            w1 += t1;
            w2 += t2;
          }
          const int y = yb + p - BS;
          if (writer) {
            const float a = static_cast<float>(w0) * 0.5f, b = static_cast<float>(w1);
            const float c = static_cast<float>(w2) * 0.5f;
            const float e = (a + c) - sqrtf((a - c) * (a - c) + b * b);
            eig[static_cast<size_t>(y) * n + x] = e;
            if (y >= band.lo && y < band.hi && px_allowed(clean, m, n, x, y, buffer_mask, any_nan))
              best = fmaxf(best, fmaxf(e, 0.f));
          }
        }
      }
#pragma unroll
      for (int j = 0; j < BS; ++j) raw[j] = nxt[j];
    }
  }
  best = wave_max(best);
  if (lane == 0) red[wave] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int b = blockIdx.y * gridDim.x + blockIdx.x;
    const float b_max = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    if (slots) {
      slot_max(slots, kSlEig, b, b_max);
    } else {
      partial[b] = b_max;
    }
  }
}

// ---- response + 3x3 non-maximum suppression + compaction in ONE pass (the resident estimate) ---------------
// lk_corner_response_cols writes the response plane (64 MiB at 4096^2) and lk_corner_select reads it back to find
// the local maxima above quality x maximum - 70 + 50 us of the estimate's critical path.  The 3x3 test does not
// need the maximum: max3x3(threshold(e)) == e and e > thr  <=>  e is a 3x3 maximum and e > thr (the threshold is
// monotone).  So the column walk judges its own rows - the last three response rows live in registers, the
// horizontal neighbours come from the adjacent lanes -, emits every positive 3x3 maximum that the NaN buffer
// allows as a candidate key, and the ordering kernels, which bin the keys by value anyway, drop what is not above
// the threshold (key_range: strictly above).  The response plane is never written.
//  * geometry: a wave computes the response for crn_cols(BS) columns and ROWS + 2 rows and judges the inner
//    crn_cols - 2 columns and ROWS rows (strip stride crn_cols - 2: 3.5 % more columns, 6 % more rows);
//  * weak maxima are dropped on the way: a candidate has to exceed quality x (the largest response the wave knows of:
//    what the finished workgroups have published in the slots when it starts, and its own strip's maximum, folded
//    over the lanes every 8 rows) - a lower bound of the final threshold, so nothing that counts is lost;
//  * no counter in the common case: wave w of the launch owns kNmsKeys slots of the output, fills them with its keys
//    and ZERO keys (which every consumer ignores: they lie below any key range) - the consumers read
//    gridDim x 4 x kNmsKeys slots (+ the overflow count: a wave with more candidates appends the rest behind the fixed
//    part through the counter word of the frame's statistic slots);
//  * the maximum goes through the kSlEig slots as before; the ordering kernels fold them themselves
//    (lk_sparse.hip load_eig_max) and corner_order writes stats[kEigMax] (lk_corner_select did that).
constexpr int kNmsKeys = 64;  // output slots per wave

using CornerKeyT = unsigned long long;
__device__ __forceinline__ CornerKeyT nms_key(float val, unsigned addr) {
  return (static_cast<CornerKeyT>(__float_as_uint(val)) << 32) | addr;
}
__device__ __forceinline__ float prev_lane_f(float v) {  // lane i gets lane i - 1's value (lane 0: 0)
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138 /* wave_shr:1 */, 0xf, 0xf, true));
}

template <int BS, int ROWS>
__global__ __launch_bounds__(256) void lk_corner_response_nms(
    const unsigned char *__restrict__ u8, const float *__restrict__ clean, int m, int n, int buffer_mask,
    const float *__restrict__ stats, float quality, CornerKeyT *__restrict__ out, int cap, Band band,
    unsigned *__restrict__ slots, int *__restrict__ zero_b, int count_b) {
  constexpr int r = BS / 2, H = r + 1, W = crn_cols(BS);
  if (blockIdx.x == 0 && blockIdx.y == 0)
    for (int i = threadIdx.x; i < count_b; i += 256) zero_b[i] = 0;  // scratch of the ordering kernels
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int *over_count = reinterpret_cast<int *>(slots + kSlCand * kSlots);
  const int fixed_total = static_cast<int>(gridDim.x * gridDim.y) * 4 * kNmsKeys;  // slots owned by the waves
  const int my_slots = (static_cast<int>(blockIdx.y * gridDim.x + blockIdx.x) * 4 + wave) * kNmsKeys;
  const int x0 = blockIdx.x * (W - 2) - 1;            // first response column of the strip
  const int yj = (blockIdx.y * 4 + wave) * ROWS;       // first JUDGED row of the wave
  const int yb = yj - 1;                               // first response row
  float best = 0.f;
  // what the finished workgroups know of the maximum (the slots hold order-preserving keys; zero = nothing yet)
  float known = fmaxf(slots_max(slots, kSlEig), 0.f);
  int held = 0;  // keys this wave has written to its slots (uniform)
  if (yj < m) {
    const float s = 1.0f / (4.0f * static_cast<float>(BS) * 255.0f), s2 = 2.f * s;
    const int xl = x0 - H + lane;  // column this lane loads; its products belong to column xl + 1
    const bool neg_x = walk_mirrored(xl + 1, n);
    const float sx = neg_x ? -s : s, sx2 = neg_x ? -s2 : s2;
    const unsigned char *col = u8 + reflect101(xl, n);
    // (the preload reaches row m + 3 BS - r - 1 here: one response row more than lk_corner_response_cols)
    constexpr int kFewRows = 2 * H + 4 > 3 * BS - r + 1 ? 2 * H + 4 : 3 * BS - r + 1;
    const bool few_rows = m < kFewRows;
    auto row_of = [&](int y) -> int {
      if (few_rows) return reflect101(y, m);
      y = y < 0 ? -y : y;
      return y >= m ? 2 * m - 2 - y : y;
    };
    auto load_row = [&](int i) -> int { return col[static_cast<size_t>(row_of(yb - H + i)) * n]; };
    auto row_terms = [&](int raw, float &hd, float &g) {
      const float a = static_cast<float>(raw);
      const float c = next_lane_f(a);
      const float b = next_lane_f(c);
      hd = b - a;
      g = (a + b) * s + c * s2;
    };
    const bool any_nan = stats[kNanCount] > 0.f;
    const int x = x0 + lane;  // response column of the lane
    const bool in_image_col = lane < W && x >= 0 && x < n;
    const bool judged_col = lane >= 1 && lane < W - 1 && x >= 1 && x < n - 1;
    const int rows_e = min(ROWS + 2, m - yb);  // response rows yb .. yb + rows_e - 1 (row m is never needed)
    const int last_p = rows_e + BS - 1;
    double ring[3][BS], V[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < BS; ++j) ring[0][j] = ring[1][j] = ring[2][j] = 0.0;
    int raw[BS];
    const int raw0 = load_row(0), raw1 = load_row(1);
#pragma unroll
    for (int j = 0; j < BS; ++j) raw[j] = load_row(2 + j);
    float hd_m, hd_0, g_m, g_0;
    row_terms(raw0, hd_m, g_m);
    row_terms(raw1, hd_0, g_0);
    // the two response rows above the newest one: value, max(left, right), max of the three
    float c1 = 0.f, h1 = 0.f, t1 = 0.f, t2 = 0.f;
    for (int base = 1; base <= last_p; base += BS) {
      int nxt[BS];
#pragma unroll
      for (int j = 0; j < BS; ++j) nxt[j] = load_row(base + BS + 1 + j);
#pragma unroll
      for (int j = 0; j < BS; ++j) {
        const int p = base + j;
        if (p > last_p) break;  // (uniform)
        constexpr int kRingBase = 1;
        const int slot = (kRingBase + j) % BS;
        float hd_p, g_p;
        row_terms(raw[j], hd_p, g_p);
        const float dx = (hd_m + hd_p) * sx + hd_0 * sx2;
        float dy = g_p - g_m;
        const int y_seq = yb - H + p;
        const bool row_mirrored = few_rows ? walk_mirrored(y_seq, m) : (y_seq < 0 || y_seq >= m);
        const unsigned row_sign = row_mirrored ? 0x80000000u : 0u;
        dy = __uint_as_float(__float_as_uint(dy) ^ row_sign);
        const double pxx = static_cast<double>(dx * dx), pxy = static_cast<double>(dx * dy);
        const double pyy = static_cast<double>(dy * dy);
        V[0] += pxx - ring[0][slot];
        V[1] += pxy - ring[1][slot];
        V[2] += pyy - ring[2][slot];
        ring[0][slot] = pxx;
        ring[1][slot] = pxy;
        ring[2][slot] = pyy;
        hd_m = hd_0;
        hd_0 = hd_p;
        g_m = g_0;
        g_0 = g_p;
        if (p >= BS) {
          double w0 = V[0], w1 = V[1], w2 = V[2];
          double q0 = V[0], q1 = V[1], q2 = V[2];
#pragma unroll
          for (int c = 0; c < 2 * r; ++c) {
            q0 = next_lane_d(q0);
            q1 = next_lane_d(q1);
            q2 = next_lane_d(q2);
            w0 += q0;
            w1 += q1;
            w2 += q2;
          }
          const int y = yb + p - BS;  // response row (>= -1)
          const float a = static_cast<float>(w0) * 0.5f, b = static_cast<float>(w1);
          const float c = static_cast<float>(w2) * 0.5f;
          const float e = (a + c) - sqrtf((a - c) * (a - c) + b * b);
          if (in_image_col && y >= 0 && y >= band.lo && y < band.hi && px_allowed(clean, m, n, x, y, buffer_mask, any_nan))
            best = fmaxf(best, fmaxf(e, 0.f));
          if ((p & 7) == 0) known = fmaxf(known, wave_max(best));  // (uniform) the strip's maximum so far
          // the row's horizontal neighbours, and the judgement of the row ABOVE it (y - 1) now that its three rows are here
          const float h0 = fmaxf(prev_lane_f(e), next_lane_f(e)), t0 = fmaxf(e, h0);
          const int yr = y - 1;
          if (p >= BS + 2 && yr >= yj) {  // (uniform) response rows y - 2, y - 1, y of this wave exist
            bool keep = judged_col && yr >= 1 && yr < m - 1 && yr >= band.lo && yr < band.hi;
            keep = keep && c1 > 0.f && c1 > known * quality;          // (> the final threshold is the ordering kernels' test)
            keep = keep && !(fmaxf(h1, fmaxf(t2, t0)) > c1);          // the 3x3 maximum
            keep = keep && px_allowed(clean, m, n, x, yr, buffer_mask, any_nan);
            const unsigned long long mask = __ballot(keep);
            if (mask != 0ull) {  // (uniform)
              const int cnt = __popcll(mask);
              int at = held + __popcll(mask & ((1ull << lane) - 1ull));
              if (held + cnt > kNmsKeys) {  // (uniform, rare) what does not fit the wave's slots goes behind the fixed part
                int base = 0;
                const int spill = held + cnt - max(held, kNmsKeys);
                if (lane == 0) base = atomicAdd(over_count, spill);
                base = __shfl(base, 0);
                if (at >= kNmsKeys) at = fixed_total + base + (at - max(held, kNmsKeys)) - my_slots;
              }
              if (keep && my_slots + at < cap) out[my_slots + at] = nms_key(c1, static_cast<unsigned>(yr + band.y_org) * n + x);
              held += cnt;
            }
          }
          t2 = t1;
          t1 = t0;
          h1 = h0;
          c1 = e;
        }
      }
#pragma unroll
      for (int j = 0; j < BS; ++j) raw[j] = nxt[j];
    }
  }
  // the rest of the wave's slots: zero keys
  for (int i = min(held, kNmsKeys) + lane; i < kNmsKeys; i += 64)
    if (my_slots + i < cap) out[my_slots + i] = 0ull;
  best = wave_max(best);
  if (lane == 0) red[wave] = best;
  __syncthreads();
  if (threadIdx.x == 0)
    slot_max(slots, kSlEig, blockIdx.y * gridDim.x + blockIdx.x, fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])));
}

// (zero_a / zero_b: counters and scratch the NEXT kernels expect cleared - done here, by a kernel
// that is a single idle-ish block anyway, instead of one 5 us fill launch each)
__global__ __launch_bounds__(kFinalThreads) void lk_max_final(const float *__restrict__ partial,
                                                              int nb, float *__restrict__ stats,
                                                              int slot, int *__restrict__ zero_a, int count_a,
                                                              int *__restrict__ zero_b, int count_b) {
  __shared__ float smem[16];
  for (int i = threadIdx.x; i < count_a; i += blockDim.x) zero_a[i] = 0;
  for (int i = threadIdx.x; i < count_b; i += blockDim.x) zero_b[i] = 0;
  float a = -INFINITY;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) a = fmaxf(a, partial[i]);
  a = block_reduce<Red::kMax>(a, smem);
  if (threadIdx.x == 0) stats[slot] = a;
}

// ---- corner candidates: threshold, 3x3 non-maximum suppression, compaction ------
// candidate key: response bits in the high word (responses are positive, so the bit pattern
// orders like the value), pixel address y*n + x in the low word; descending key order is the
// order goodFeaturesToTrack walks the corners in (strongest first, ties: higher address first)
using CornerKey = unsigned long long;
__host__ __device__ inline CornerKey make_corner_key(float val, unsigned addr) {
#if defined(__HIP_DEVICE_COMPILE__)
  const unsigned bits = __float_as_uint(val);
#else
  unsigned bits;
  std::memcpy(&bits, &val, sizeof(bits));
#endif
  return (static_cast<CornerKey>(bits) << 32) | addr;
}

// A workgroup of kSelWaves waves covers 256 rows x 62 columns (kSelWide = 0: the waves stacked vertically) or 64 rows x
// 248 columns (kSelWide = 1: side by side - a workgroup's row loads are 1 KiB of consecutive addresses instead of four
// 256-byte pieces 64 rows apart); every wave works through kSelGroups groups of 16 rows; one reservation of output per
// workgroup (see below).  Round 6 measured 16 waves x 1 group at the same coverage (four times the loads in flight):
// 68 us against 54 at 4096^2, LK leg 0.596 against 0.580 ms (profiles/r06/g_select_16x1_ab.txt) - the pass is not
// short of loads in flight.
#ifndef PSH_SEL_WAVES
#define PSH_SEL_WAVES 4
#endif
#ifndef PSH_SEL_GROUPS
#define PSH_SEL_GROUPS 4
#endif
#ifndef PSH_SEL_WIDE
#define PSH_SEL_WIDE 1
#endif
constexpr int kSelWaves = PSH_SEL_WAVES;
constexpr int kSelGroups = PSH_SEL_GROUPS;   // 16-row groups a wave works through
constexpr bool kSelWide = PSH_SEL_WIDE != 0;
constexpr int kSelCols = 62;                 // columns per wave: 64 lanes minus one halo column on each side
constexpr int kSelWgRows = kSelWide ? 16 * kSelGroups : 16 * kSelGroups * kSelWaves;  // rows / columns of a workgroup
constexpr int kSelWgCols = kSelWide ? kSelCols * kSelWaves : kSelCols;

// A wave owns 62 columns and works through four groups of 16 rows: for each it loads the 18 rows
// of the response it needs (all loads in flight together), takes the left / right neighbours from
// the adjacent lanes and the rows above / below from its own registers - the 3x3 maximum test never
// goes back to memory.  The candidates' masks wait in LDS until the workgroup has reserved its
// output range with ONE atomic: a single global counter takes ~90 atomics per microsecond, which is
// what bounded the kernel while a workgroup covered 64 x 64 pixels (4096 atomics = 46 us at 4096^2,
// whatever the kernel did otherwise).
__global__ __launch_bounds__(64 * kSelWaves) void lk_corner_select(const float *__restrict__ eig,
                                                        const float *__restrict__ clean, int m,
                                                        int n, int buffer_mask, float quality,
                                                        float *__restrict__ stats,
                                                        CornerKey *__restrict__ out, int cap,
                                                        int *__restrict__ count, Band band,
                                                        const unsigned *__restrict__ slots) {
  constexpr int kRows = 16;  // rows per group
  __shared__ unsigned long long s_mask[kSelWaves][kSelGroups * kRows];
  __shared__ int wave_count[kSelWaves];
  __shared__ int block_base;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // lane l LOADS column x0 - 1 + l and JUDGES the column to its right, xc = x0 + l: its own value is the
  // left neighbour, the centre and the right neighbour come from lanes l + 1 and l + 2 (DPP wave_shl
  // moves, 4 cycles each; the ds_bpermute behind __shfl_up / __shfl_down costs 24)
  const int x = (kSelWide ? (blockIdx.x * kSelWaves + wave) : blockIdx.x) * kSelCols - 1 + lane, xc = x + 1;
  const int y_wave = (kSelWide ? blockIdx.y : (blockIdx.y * kSelWaves + wave)) * (kSelGroups * kRows);
  // slots != nullptr: the maximum response comes from the statistic slots (the response pass wrote them)
  // and workgroup (0, 0) writes it into stats[] for the ordering kernels
  const float eig_max = slots ? slots_max(slots, kSlEig) : stats[kEigMax];
  if (slots && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) stats[kEigMax] = eig_max;
  const float thr = eig_max * quality;
  const bool any_nan = stats[kNanCount] > 0.f;
  const bool col_in = x >= 0 && x < n;
  const bool col_ok = lane < kSelCols && xc >= 1 && xc < n - 1;
  int mine = 0;
  for (int g = 0; g < kSelGroups; ++g) {
    const int y_first = y_wave + g * kRows;
    if (y_first >= m) {  // (uniform) nothing below the image
      if (lane < kRows) s_mask[wave][g * kRows + lane] = 0ull;
      continue;
    }
    float v[kRows + 2], m3[kRows + 2], hmax[kRows + 2];
#pragma unroll
    for (int q = 0; q < kRows + 2; ++q) {
      const int y = y_first - 1 + q;
      v[q] = (col_in && y >= 0 && y < m) ? eig[static_cast<size_t>(y) * n + x] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < kRows + 2; ++q) {
      const float left = v[q], centre = next_lane_f(left), right = next_lane_f(centre);
      hmax[q] = fmaxf(left, right);
      m3[q] = fmaxf(centre, hmax[q]);
      v[q] = centre;
    }
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
      const int yr = y_first + r;
      const float c = v[r + 1];
      bool keep = col_ok && yr >= 1 && yr < m - 1 && yr >= band.lo && yr < band.hi;
      keep = keep && c > thr && c != 0.f;                                 // THRESH_TOZERO keeps values > thr
      keep = keep && !(fmaxf(hmax[r + 1], fmaxf(m3[r], m3[r + 2])) > c);  // the 3x3 maximum
      keep = keep && px_allowed(clean, m, n, xc, yr, buffer_mask, any_nan);
      const unsigned long long mask = __ballot(keep);
      if (lane == 0) s_mask[wave][g * kRows + r] = mask;
      mine += __popcll(mask);
    }
  }
  if (lane == 0) wave_count[wave] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
    for (int w = 0; w < kSelWaves; ++w) total += wave_count[w];
    block_base = total > 0 ? atomicAdd(count, total) : 0;
  }
  __syncthreads();
  int pos = block_base;
  for (int w = 0; w < wave; ++w) pos += wave_count[w];
  if (mine == 0) return;
  // pass 2: the kept pixels get their destination (their responses are read again: a few per row)
  for (int r = 0; r < kSelGroups * kRows; ++r) {
    const unsigned long long mask = s_mask[wave][r];
    if (mask == 0ull) continue;
    const int y = y_wave + r;
    if ((mask >> lane) & 1ull) {
      const int at = pos + __popcll(mask & ((1ull << lane) - 1ull));
      if (at < cap)
        out[at] = make_corner_key(eig[static_cast<size_t>(y) * n + xc], static_cast<unsigned>(y + band.y_org) * n + xc);
    }
    pos += __popcll(mask);
  }
}

// ---- Gaussian pyramid level: cv::pyrDown for 8U ---------------------------------
// out(oy, ox) = (sum_{i,j} w_i w_j src(2 oy + i - 2, 2 ox + j - 2) + 128) >> 8, w = [1 4 6 4 1], reflect-101.
// (Rounds 1-3: a 32 x 8 tile through LDS with five byte loads per filtered value - 0.06 of the HBM
// rate.)  A lane owns FOUR adjacent output columns and walks kPyrRows output rows: per input row it
// loads the 16 bytes [2 ox - 4, 2 ox + 12) with ONE dwordx4 (the eleven taps of its four outputs sit at
// bytes 2 .. 12), filters them horizontally in registers, keeps the last rows' sums for the vertical
// filter and stores one dword per output row; all rows of a half are loaded before the first is used.
// Lanes whose window leaves the image (the first and the last few columns) or an image whose rows are
// not dword-aligned assemble the window from byte loads at reflected columns.  Both images of a
// pair in one launch (blockIdx.z).
constexpr int kPyrRows = 8;  // output rows per wave: 2 * 8 + 3 input rows

struct PyrPair {
  const unsigned char *src[2];
  unsigned char *dst[2];
};

// kPyrRows output rows of one lane's four columns.  FAST: one dwordx4 per input row; otherwise the same 16
// bytes are assembled from eleven byte loads at the reflected columns off[] (the same for every row).  The
// two routes are separate straight-line bodies: a branch per row would put a wait behind every load
template <bool FAST>
__device__ __forceinline__ void pyr_rows(const unsigned char *__restrict__ src, unsigned char *__restrict__ dst, int m,
                                         int n, int om, int on, int ox, int oy0, int wx, const int (&off)[11]) {
  auto window = [&](const unsigned char *row) -> uint4 {
    if (FAST) return *reinterpret_cast<const uint4 *>(row + wx);
    unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 11; ++k) w[(k + 2) >> 2] |= static_cast<unsigned>(row[off[k]]) << (8 * ((k + 2) & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
  };
  auto hrow = [&](const uint4 d, int h[4]) {
    // bytes 2 .. 12 of the window: b[k] = byte k + 2
    const unsigned w[4] = {d.x, d.y, d.z, d.w};
    auto b = [&](int k) -> int { return static_cast<int>((w[(k + 2) >> 2] >> (8 * ((k + 2) & 3))) & 0xffu); };
#pragma unroll
    for (int j = 0; j < 4; ++j) h[j] = b(2 * j) + b(2 * j + 4) + 4 * (b(2 * j + 1) + b(2 * j + 3)) + 6 * b(2 * j + 2);
  };
  auto row_ptr = [&](int y) { return src + static_cast<size_t>(reflect101(y, m)) * n; };  // (scalar)
  const bool store4 = (on & 3) == 0 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0 && ox + 3 < on;
  constexpr int kHalf = kPyrRows / 2, kIn = 2 * kHalf + 3;
  int h[kIn][4];  // horizontally filtered rows of one half: 4 output rows need 11
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const int oyh = oy0 + half * kHalf;
    if (oyh >= om) break;  // (uniform)
    // rows 2 oyh - 2 .. 2 oyh + 2 kHalf: the first three are the last three of the previous half
    const int keep = half == 0 ? 0 : 3;
    if (half != 0) {
#pragma unroll
      for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) h[q][j] = h[kIn - 3 + q][j];
    }
    uint4 d[kIn];
#pragma unroll
    for (int q = keep; q < kIn; ++q) d[q] = window(row_ptr(2 * oyh - 2 + q));
#pragma unroll
    for (int q = keep; q < kIn; ++q) hrow(d[q], h[q]);
#pragma unroll
    for (int i = 0; i < kHalf; ++i) {
      const int oy = oyh + i;
      if (oy >= om) break;  // (uniform)
      unsigned packed = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int v = h[2 * i][j] + 4 * h[2 * i + 1][j] + 6 * h[2 * i + 2][j] + 4 * h[2 * i + 3][j] + h[2 * i + 4][j];
        packed |= static_cast<unsigned>((v + 128) >> 8) << (8 * j);
      }
      unsigned char *out = dst + static_cast<size_t>(oy) * on + ox;
      if (store4) {
        *reinterpret_cast<unsigned *>(out) = packed;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (ox + j < on) out[j] = static_cast<unsigned char>(packed >> (8 * j));
      }
    }
  }
}

__global__ __launch_bounds__(256) void lk_pyrdown(PyrPair pair, int m, int n, int om, int on) {
  const unsigned char *__restrict__ src = pair.src[blockIdx.z];
  unsigned char *__restrict__ dst = pair.dst[blockIdx.z];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ox = (blockIdx.x * 64 + lane) * 4;  // first of the lane's output columns
  const int oy0 = (blockIdx.y * 4 + wave) * kPyrRows;
  if (oy0 >= om) return;  // (uniform; no barrier below)
  const int wx = 2 * ox - 4;  // first byte of the 16-byte window
  const bool rows_aligned = (n & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 3) == 0;
  const bool fast = rows_aligned && wx >= 0 && wx + 16 <= n;
  int off[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (fast) {
    pyr_rows<true>(src, dst, m, n, om, on, ox, oy0, wx, off);
  } else if (ox < on) {
    // columns >= on are never stored, their taps only have to stay inside the row
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      int i = wx + 2 + k;
      if (n < 16) {
        i = reflect101(i, n);
      } else {
        i = i < 0 ? -i : i;
        i = i >= n ? 2 * n - 2 - i : i;
        i = min(max(i, 0), n - 1);
      }
      off[k] = i;
    }
    pyr_rows<false>(src, dst, m, n, om, on, ox, oy0, wx, off);
  }
}

// ---- Scharr gradients: calcSharrDeriv, int16 (Ix, Iy) interleaved ----------------
__global__ __launch_bounds__(256) void lk_scharr(const unsigned char *__restrict__ src, int m,
                                                 int n, short2 *__restrict__ dst) {
  constexpr int TX = 64, TY = 4;
  __shared__ short tile[TY + 2][TX + 2];
  const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
  const int tid = threadIdx.x;
  for (int i = tid; i < (TY + 2) * (TX + 2); i += 256) {
    const int ly = i / (TX + 2), lx = i % (TX + 2);
    const int y = reflect101(y0 + ly - 1, m), x = reflect101(x0 + lx - 1, n);
    tile[ly][lx] = src[static_cast<size_t>(y) * n + x];
  }
  __syncthreads();
  const int lx = tid % TX + 1, ly = tid / TX + 1;
  const int x = x0 + lx - 1, y = y0 + ly - 1;
  if (x < n && y < m) {
    const int t0l = (tile[ly - 1][lx - 1] + tile[ly + 1][lx - 1]) * 3 + tile[ly][lx - 1] * 10;
    const int t0r = (tile[ly - 1][lx + 1] + tile[ly + 1][lx + 1]) * 3 + tile[ly][lx + 1] * 10;
    const int t1l = tile[ly + 1][lx - 1] - tile[ly - 1][lx - 1];
    const int t1c = tile[ly + 1][lx] - tile[ly - 1][lx];
    const int t1r = tile[ly + 1][lx + 1] - tile[ly - 1][lx + 1];
    dst[static_cast<size_t>(y) * n + x] =
        make_short2(static_cast<short>(t0r - t0l), static_cast<short>((t1r + t1l) * 3 + t1c * 10));
  }
}

// ---- pyramidal LK tracker: LKTrackerInvoker, one workgroup per feature ------------
constexpr int kMaxLevels = 8;
constexpr int kMaxWin = 64;

struct PyrLevel {
  const unsigned char *I, *J;  // previous / next frame at this level
  const short2 *dI;            // Scharr gradients of I
  int rows, cols;
  // rows [vlo, vhi) hold the values the pyramid of the WHOLE frame has there.  Whole frames:
  // everything; row bands processed as sub-images (multi-GPU tiling): all but a margin at the edges
  // that are not frame borders.  A track whose windows leave that range is marked (status bit 1)
  // and redone on whole-frame data by the caller.
  int vlo = -(1 << 30), vhi = 1 << 30;
  // band pyramids store the rows [row_org, row_org + rows_stored) of the level only; `rows` stays
  // the height of the whole level, so that positions, reflections and border tests are computed
  // in whole-frame coordinates (float positions round by their magnitude: shifting the origin
  // would change low-order bits of the tracks)
  int row_org = 0, rows_stored = 1 << 30;
};
// offset of (whole-level) row y in the stored rows; rows outside the band are clamped (such
// accesses are marked through vlo / vhi, they only must not leave the allocation)
__device__ __forceinline__ size_t stored_row(const PyrLevel &L, int y) {
  return static_cast<size_t>(min(max(y - L.row_org, 0), L.rows_stored - 1));
}
struct Pyramid {
  PyrLevel lv[kMaxLevels];
  int top;  // index of the coarsest level
};

__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// Sum over the wave of a value that fits 32 bits per lane (|v| < 2^31), exact in 64 bits, delivered
// to every lane.  The 64-bit sum through __shfl_xor is 12 ds_bpermute round trips (24 cycles each,
// profiles/r04/a_valu_probe.txt); here the value is split into its low 16 bits and the rest, each half
// is summed in 32 bits by six DPP steps (4 cycles each: <= 64 x 2^16 cannot overflow), and the halves
// are put together once.
__device__ __forceinline__ int wave_sum_dpp_i32(int v) {
#define PSH_SUM_STEP(CTRL, ROWMASK) v += __builtin_amdgcn_update_dpp(0, v, CTRL, ROWMASK, 0xf, false);
  PSH_SUM_STEP(0xB1, 0xf)   // quad_perm:[1,0,3,2]
  PSH_SUM_STEP(0x4E, 0xf)   // quad_perm:[2,3,0,1]
  PSH_SUM_STEP(0x141, 0xf)  // row_half_mirror
  PSH_SUM_STEP(0x140, 0xf)  // row_mirror
  PSH_SUM_STEP(0x142, 0xa)  // row_bcast:15 -> rows 1 and 3
  PSH_SUM_STEP(0x143, 0xc)  // row_bcast:31 -> rows 2 and 3
#undef PSH_SUM_STEP
  return __builtin_amdgcn_readlane(v, 63);
}
__device__ __forceinline__ long long wave_sum_split_i64(int v) {
  const int lo = wave_sum_dpp_i32(v & 0xffff), hi = wave_sum_dpp_i32(v >> 16);
  return (static_cast<long long>(hi) << 16) + lo;
}

__device__ __forceinline__ void lk_weights(float a, float b, int &w00, int &w01, int &w10, int &w11) {
  const float s = 16384.f;  // 1 << W_BITS
  w00 = static_cast<int>(rintf((1.f - a) * (1.f - b) * s));  // cvRound: half to even
  w01 = static_cast<int>(rintf(a * (1.f - b) * s));
  w10 = static_cast<int>(rintf((1.f - a) * b * s));
  w11 = 16384 - w00 - w01 - w10;
}

__device__ __forceinline__ int descale(int v, int n) { return (v + (1 << (n - 1))) >> n; }
// a w00 + b w01 + c w10 + d w11 for factors of at most 24 bits (signed): same integer result as the
// 32-bit products, on the full-rate 24-bit multiplier
__device__ __forceinline__ int bilin24(int a, int b, int c, int d, int w00, int w01, int w10, int w11) {
  return __mul24(a, w00) + __mul24(b, w01) + __mul24(c, w10) + __mul24(d, w11);
}

// kPer: window samples per thread, >= ceil(win_w * win_h / 256) (4, 10 or 16: 32x32, 50x50, 64x64)
template <int kPer>
__global__ __launch_bounds__(256) void lk_track(Pyramid pyr, const float2 *__restrict__ pts,
                                                int npts, const int *__restrict__ npts_dev, int win_w,
                                                int win_h, int max_count, float eps2, float min_eig_thr,
                                                float2 *__restrict__ next_pts,
                                                unsigned char *__restrict__ status) {
  __shared__ short sI[kMaxWin * kMaxWin];
  __shared__ short sGx[kMaxWin * kMaxWin];
  __shared__ short sGy[kMaxWin * kMaxWin];
  __shared__ long long red[3][4];
  const int p = blockIdx.x;
  // the point count is either a launch argument or still in device memory (corner_order's output;
  // the grid then covers the capacity and the surplus workgroups leave at once)
  if (npts_dev) npts = min(npts, *npts_dev);
  if (p >= npts) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int area = win_w * win_h;
  const float half_x = (win_w - 1) * 0.5f, half_y = (win_h - 1) * 0.5f;
  const float2 pt = pts[p];
  float nx = 0.f, ny = 0.f;  // tracked position (with half window added back)
  bool ok = true, suspect = false;
  // window samples of this thread (the same on every level and iteration): sample i = tid + 256 q
  int wxs[kPer], wys[kPer];
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
    const int i = min(tid + 256 * q, area - 1);
    wys[q] = i / win_w;
    wxs[q] = i - wys[q] * win_w;
  }

  for (int level = pyr.top; level >= 0; --level) {
    const PyrLevel L = pyr.lv[level];
    const float scale = 1.f / static_cast<float>(1 << level);
    float px = pt.x * scale, py = pt.y * scale;
    if (level == pyr.top) {
      nx = px;
      ny = py;
    } else {
      nx *= 2.f;
      ny *= 2.f;
    }
    px -= half_x;
    py -= half_y;
    const int ipx = static_cast<int>(floorf(px)), ipy = static_cast<int>(floorf(py));
    if (ipy - 1 < L.vlo || ipy + win_h + 2 > L.vhi) suspect = true;
    if (ipx < -win_w || ipx >= L.cols || ipy < -win_h || ipy >= L.rows) {
      if (level == 0) ok = false;
      continue;
    }
    int w00, w01, w10, w11;
    lk_weights(px - static_cast<float>(ipx), py - static_cast<float>(ipy), w00, w01, w10, w11);
    // ---- template patch + spatial gradient matrix -------------------------------
    // per-thread partial sums fit 32 bits: |g| <= 16 * 255, <= 16 samples per thread
    int s11 = 0, s12 = 0, s22 = 0;
    __syncthreads();  // previous level's readers are done with the LDS patch
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      const int i = tid + 256 * q;
      if (i < area) {
        const int x = ipx + wxs[q], y = ipy + wys[q];
        // image taps: reflect-101 padding; gradient taps: zero outside the image
        const int xa = reflect101(x, L.cols), xb = reflect101(x + 1, L.cols);
        const int ya = reflect101(y, L.rows), yb = reflect101(y + 1, L.rows);
        const unsigned char *ra = L.I + stored_row(L, ya) * L.cols;
        const unsigned char *rb = L.I + stored_row(L, yb) * L.cols;
        const int ival = descale(ra[xa] * w00 + ra[xb] * w01 + rb[xa] * w10 + rb[xb] * w11, 14 - 5);
        const bool x_in0 = x >= 0 && x < L.cols, x_in1 = x + 1 >= 0 && x + 1 < L.cols;
        const bool y_in0 = y >= 0 && y < L.rows, y_in1 = y + 1 >= 0 && y + 1 < L.rows;
        const short2 z = make_short2(0, 0);
        const short2 g00 = (x_in0 && y_in0) ? L.dI[stored_row(L, y) * L.cols + x] : z;
        const short2 g01 = (x_in1 && y_in0) ? L.dI[stored_row(L, y) * L.cols + x + 1] : z;
        const short2 g10 = (x_in0 && y_in1) ? L.dI[stored_row(L, y + 1) * L.cols + x] : z;
        const short2 g11 = (x_in1 && y_in1) ? L.dI[stored_row(L, y + 1) * L.cols + x + 1] : z;
        const int gx = descale(g00.x * w00 + g01.x * w01 + g10.x * w10 + g11.x * w11, 14);
        const int gy = descale(g00.y * w00 + g01.y * w01 + g10.y * w10 + g11.y * w11, 14);
        sI[i] = static_cast<short>(ival);
        sGx[i] = static_cast<short>(gx);
        sGy[i] = static_cast<short>(gy);
        s11 += gx * gx;
        s12 += gx * gy;
        s22 += gy * gy;
      }
    }
    long long a11 = s11, a12 = s12, a22 = s22;
    a11 = wave_sum_i64(a11);
    a12 = wave_sum_i64(a12);
    a22 = wave_sum_i64(a22);
    if (lane == 0) {
      red[0][wave] = a11;
      red[1][wave] = a12;
      red[2][wave] = a22;
    }
    __syncthreads();
    const float flt_scale = 1.f / 1048576.f;  // 2^-20
    const float A11 = static_cast<float>(red[0][0] + red[0][1] + red[0][2] + red[0][3]) * flt_scale;
    const float A12 = static_cast<float>(red[1][0] + red[1][1] + red[1][2] + red[1][3]) * flt_scale;
    const float A22 = static_cast<float>(red[2][0] + red[2][1] + red[2][2] + red[2][3]) * flt_scale;
    float D = A11 * A22 - A12 * A12;
    const float min_eig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) /
                          static_cast<float>(2 * win_w * win_h);
    if (min_eig < min_eig_thr || D < 1.1920929e-07f) {
      if (level == 0) ok = false;
      continue;
    }
    D = 1.f / D;
    float qx = nx - half_x, qy = ny - half_y;
    float prev_dx = 0.f, prev_dy = 0.f;
    for (int j = 0; j < max_count; ++j) {
      const int inx = static_cast<int>(floorf(qx)), iny = static_cast<int>(floorf(qy));
      if (iny < L.vlo || iny + win_h + 1 > L.vhi) suspect = true;
      if (inx < -win_w || inx >= L.cols || iny < -win_h || iny >= L.rows) {
        if (level == 0) ok = false;
        break;
      }
      lk_weights(qx - static_cast<float>(inx), qy - static_cast<float>(iny), w00, w01, w10, w11);
      // all taps of the thread's samples are requested before any is used: one memory round
      // trip per iteration instead of one per sample
      int t00[kPer], t01[kPer], t10[kPer], t11[kPer];
#pragma unroll
      for (int q = 0; q < kPer; ++q) {  // (samples past the window repeat its last one, unused)
        const int x = inx + wxs[q], y = iny + wys[q];
        const int xa = reflect101(x, L.cols), xb = reflect101(x + 1, L.cols);
        const int ya = reflect101(y, L.rows), yb = reflect101(y + 1, L.rows);
        const unsigned char *ra = L.J + stored_row(L, ya) * L.cols;
        const unsigned char *rb = L.J + stored_row(L, yb) * L.cols;
        t00[q] = ra[xa];
        t01[q] = ra[xb];
        t10[q] = rb[xa];
        t11[q] = rb[xb];
      }
      int c1 = 0, c2 = 0;  // |diff * g| < 2^26, <= 16 samples per thread
#pragma unroll
      for (int q = 0; q < kPer; ++q) {
        const int i = tid + 256 * q;
        if (i < area) {
          const int diff = descale(t00[q] * w00 + t01[q] * w01 + t10[q] * w10 + t11[q] * w11, 14 - 5) - sI[i];
          c1 += diff * sGx[i];
          c2 += diff * sGy[i];
        }
      }
      long long b1 = c1, b2 = c2;
      b1 = wave_sum_i64(b1);
      b2 = wave_sum_i64(b2);
      __syncthreads();  // everyone has consumed the previous reduction
      if (lane == 0) {
        red[0][wave] = b1;
        red[1][wave] = b2;
      }
      __syncthreads();
      const float B1 = static_cast<float>(red[0][0] + red[0][1] + red[0][2] + red[0][3]) * flt_scale;
      const float B2 = static_cast<float>(red[1][0] + red[1][1] + red[1][2] + red[1][3]) * flt_scale;
      const float dx = (A12 * B2 - A22 * B1) * D;
      const float dy = (A12 * B1 - A11 * B2) * D;
      qx += dx;
      qy += dy;
      nx = qx + half_x;
      ny = qy + half_y;
      if (dx * dx + dy * dy <= eps2) break;
      if (j > 0 && fabsf(dx + prev_dx) < 0.01f && fabsf(dy + prev_dy) < 0.01f) {
        nx -= dx * 0.5f;
        ny -= dy * 0.5f;
        break;
      }
      prev_dx = dx;
      prev_dy = dy;
    }
    if (level == 0 && ok) {
      // the Python binding always asks for the error output: the final window must
      // start inside the (padded) image, else the feature is dropped
      const int rx = static_cast<int>(rintf(nx - half_x)), ry = static_cast<int>(rintf(ny - half_y));
      if (ry < L.vlo || ry + win_h + 1 > L.vhi) suspect = true;
      if (rx < -win_w || rx >= L.cols || ry < -win_h || ry >= L.rows) ok = false;
    }
  }
  if (tid == 0) {
    next_pts[p] = make_float2(nx, ny);
    status[p] = (ok ? 1 : 0) | (suspect ? 2 : 0);
  }
}

// ---- row-structured tracker (windows up to 63 columns) ---------------------------------------
// Same arithmetic as lk_track; what changes is how the window reaches the registers.  A vector
// memory instruction costs the CU's address pipeline the same whether it gathers bytes or
// dwords (docs/history.md 3.1), and lk_track issues four byte gathers per window sample and pass.
// Here a lane owns a window COLUMN and a wave a band of ROWS window rows: every image row of
// the band is loaded once (column x by lane x - x0; lane win_w fetches the extra column), the
// right-hand tap comes from the next lane by DPP and the lower tap row is the next row's upper
// one - (ROWS + 1) loads per wave and pass instead of 4 * ROWS.
// The Scharr gradients of the template window (calcSharrDeriv: reflect-101 stencil inside the
// image, zero outside) are computed here from the same rows, so no gradient image is built at
// all: the tracker touches ~1000 windows, the full-image Scharr pass wrote 5 bytes per pixel of
// every level.
__device__ __forceinline__ int from_next_lane(int v) {
  return __builtin_amdgcn_update_dpp(0, v, 0x130 /* wave_shl:1 */, 0xf, 0xf, true);
}
constexpr int kRowsMaxWin = 61;  // window columns + 3 (Scharr halo, right tap) have to fit a wave

template <int ROWS>
__global__ __launch_bounds__(256) void lk_track_rows(Pyramid pyr, const float2 *__restrict__ pts, int npts,
                                                     const int *__restrict__ npts_dev, int win_w, int win_h,
                                                     int max_count, float eps2, float min_eig_thr,
                                                     float2 *__restrict__ next_pts,
                                                     unsigned char *__restrict__ status) {
  __shared__ long long red[3][4];
  __shared__ long long red_b[2][2][4];  // iteration sums of the four waves, two buffers in turn
  // the template patch of the lane's column - value and the two gradients of its ROWS window rows - stays
  // in registers (rounds 2-4 kept it in LDS and read it back row by row in every iteration: three reads and
  // a wait per row); rows and lanes outside the window hold zero gradients, so the iteration needs no
  // per-row branch and no execution mask
  int rI[ROWS], rGx[ROWS], rGy[ROWS];
  const int p = blockIdx.x;
  if (npts_dev) npts = min(npts, *npts_dev);  // count in device memory: see lk_track
  if (p >= npts) return;
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const float half_x = (win_w - 1) * 0.5f, half_y = (win_h - 1) * 0.5f;
  const float2 pt = pts[p];
  float nx = 0.f, ny = 0.f;  // tracked position (with half window added back)
  bool ok = true, suspect = false;
  const int row_first = wave * ROWS;                          // window rows of this wave
  const int row_count = min(ROWS, win_h - row_first);         // may be <= 0 for the last waves
  const bool sample_lane = lane < win_w;

  for (int level = pyr.top; level >= 0; --level) {
    const PyrLevel L = pyr.lv[level];
    const float scale = 1.f / static_cast<float>(1 << level);
    float px = pt.x * scale, py = pt.y * scale;
    if (level == pyr.top) {
      nx = px;
      ny = py;
    } else {
      nx *= 2.f;
      ny *= 2.f;
    }
    px -= half_x;
    py -= half_y;
    const int ipx = static_cast<int>(floorf(px)), ipy = static_cast<int>(floorf(py));
    if (ipy - 1 < L.vlo || ipy + win_h + 2 > L.vhi) suspect = true;
    if (ipx < -win_w || ipx >= L.cols || ipy < -win_h || ipy >= L.rows) {
      if (level == 0) ok = false;
      continue;
    }
    int w00, w01, w10, w11;
    lk_weights(px - static_cast<float>(ipx), py - static_cast<float>(ipy), w00, w01, w10, w11);
    // ---- template patch + spatial gradient matrix -------------------------------
    int s11 = 0, s12 = 0, s22 = 0;  // per-thread partial sums fit 32 bits (|g| <= 16 * 255)
    __syncthreads();  // previous level's readers are done with red[]
#pragma unroll
    for (int r = 0; r < ROWS; ++r) rI[r] = rGx[r] = rGy[r] = 0;
    {
      // lanes 0 .. win_w + 2 LOAD image columns ipx - 1 .. ipx + win_w + 1; everything a lane then
      // works on belongs to the column one to the right, xd = ipx + lane, assembled from lanes
      // l, l + 1, l + 2 with wave_shl DPP only (a centred form with wave_shr folded into the
      // subtraction came out with zero x-gradients on the device, although a plain
      // v_mov_b32_dpp wave_shr:1 does deliver lane l - 1: tools/dpp_probe.py)
      const int x = ipx - 1 + lane;
      const int xa = reflect101(x, L.cols);
      const int xd = ipx + lane;
      const bool xd_in = xd >= 0 && xd < L.cols;
      const bool tpl_load = lane <= win_w + 2;
      // image rows ipy + row_first - 1 ... + row_count + 1 (reflect-101), one byte per lane
      int ti[ROWS + 3];
#pragma unroll
      for (int r = 0; r < ROWS + 3; ++r) {
        ti[r] = 0;
        if (r < row_count + 3 && tpl_load)
          ti[r] = L.I[stored_row(L, reflect101(ipy + row_first - 1 + r, L.rows)) * L.cols + xa];
      }
      // Scharr gradients of column xd at rows ipy + row_first ... + row_count: (Ix, Iy) packed
      int tg[ROWS + 1];
#pragma unroll
      for (int r = 0; r <= ROWS; ++r) {
        tg[r] = 0;
        if (r <= row_count) {
          const int up = ti[r], mid = ti[r + 1], dn = ti[r + 2];
          const int t0 = (up + dn) * 3 + mid * 10, t1 = dn - up;  // column xd - 1
          const int t0_r = from_next_lane(from_next_lane(t0));     // column xd + 1
          const int t1_c = from_next_lane(t1), t1_r = from_next_lane(t1_c);
          const int gx = t0_r - t0;
          const int gy = (t1 + t1_r) * 3 + t1_c * 10;
          const int y = ipy + row_first + r;
          const bool in = xd_in && y >= 0 && y < L.rows;  // the gradient image is zero-padded
          tg[r] = in ? ((gy << 16) | (gx & 0xffff)) : 0;
        }
      }
#pragma unroll
      for (int r = 0; r < ROWS; ++r) {
        if (r < row_count) {
          const int i00 = from_next_lane(ti[r + 1]), i01 = from_next_lane(i00);
          const int i10 = from_next_lane(ti[r + 2]), i11 = from_next_lane(i10);
          const int g00 = tg[r], g01 = from_next_lane(tg[r]), g10 = tg[r + 1], g11 = from_next_lane(tg[r + 1]);
          if (sample_lane) {
            // (every factor fits 24 bits - pixels 8, gradients 14, weights 15 -: v_mad_i32_i24 runs at
            // full rate, the 32-bit v_mul_lo_u32 the compiler would pick at a quarter of it)
            const int ival = descale(bilin24(i00, i01, i10, i11, w00, w01, w10, w11), 14 - 5);
            const int gx = descale(bilin24(static_cast<short>(g00), static_cast<short>(g01), static_cast<short>(g10),
                                           static_cast<short>(g11), w00, w01, w10, w11), 14);
            const int gy = descale(bilin24(g00 >> 16, g01 >> 16, g10 >> 16, g11 >> 16, w00, w01, w10, w11), 14);
            rI[r] = static_cast<short>(ival);
            rGx[r] = static_cast<short>(gx);
            rGy[r] = static_cast<short>(gy);
            s11 += gx * gx;
            s12 += gx * gy;
            s22 += gy * gy;
          }
        }
      }
    }
    const long long a11 = wave_sum_split_i64(s11), a12 = wave_sum_split_i64(s12), a22 = wave_sum_split_i64(s22);
    if (lane == 0) {
      red[0][wave] = a11;
      red[1][wave] = a12;
      red[2][wave] = a22;
    }
    __syncthreads();
    const float flt_scale = 1.f / 1048576.f;  // 2^-20
    const float A11 = static_cast<float>(red[0][0] + red[0][1] + red[0][2] + red[0][3]) * flt_scale;
    const float A12 = static_cast<float>(red[1][0] + red[1][1] + red[1][2] + red[1][3]) * flt_scale;
    const float A22 = static_cast<float>(red[2][0] + red[2][1] + red[2][2] + red[2][3]) * flt_scale;
    float D = A11 * A22 - A12 * A12;
    const float min_eig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) /
                          static_cast<float>(2 * win_w * win_h);
    if (min_eig < min_eig_thr || D < 1.1920929e-07f) {
      if (level == 0) ok = false;
      continue;
    }
    D = 1.f / D;
    float qx = nx - half_x, qy = ny - half_y;
    float prev_dx = 0.f, prev_dy = 0.f;
    for (int j = 0; j < max_count; ++j) {
      const int inx = static_cast<int>(floorf(qx)), iny = static_cast<int>(floorf(qy));
      if (iny < L.vlo || iny + win_h + 1 > L.vhi) suspect = true;
      if (inx < -win_w || inx >= L.cols || iny < -win_h || iny >= L.rows) {
        if (level == 0) ok = false;
        break;
      }
      lk_weights(qx - static_cast<float>(inx), qy - static_cast<float>(iny), w00, w01, w10, w11);
      // image rows iny + row_first ... + ROWS of the next frame, one byte per lane and row.  As a rule the
      // whole block lies inside the (stored) image: one base address, no reflection, straight-line loads;
      // near a border every row and column is reflected (rows past the wave's share repeat its last one:
      // their gradients are zero)
      const int y0 = iny + row_first;
      const bool inside = row_count > 0 && inx >= 0 && inx + 63 < L.cols && y0 >= 0 && y0 + ROWS < L.rows &&
                          y0 >= L.row_org && y0 + ROWS - L.row_org < L.rows_stored;  // (uniform)
      int tj[ROWS + 1];
      if (inside) {
        const unsigned char *base = L.J + static_cast<size_t>(y0 - L.row_org) * L.cols + (inx + lane);
#pragma unroll
        for (int r = 0; r <= ROWS; ++r) tj[r] = base[static_cast<size_t>(r) * L.cols];
      } else {
        const int xa = reflect101(inx + lane, L.cols);
#pragma unroll
        for (int r = 0; r <= ROWS; ++r)
          tj[r] = L.J[stored_row(L, reflect101(y0 + min(r, max(row_count, 0)), L.rows)) * L.cols + xa];
      }
      int c1 = 0, c2 = 0;  // |diff * g| < 2^26, <= 16 samples per thread
      int right = from_next_lane(tj[0]);
#pragma unroll
      for (int r = 0; r < ROWS; ++r) {
        const int right_below = from_next_lane(tj[r + 1]);
        const int diff = descale(bilin24(tj[r], right, tj[r + 1], right_below, w00, w01, w10, w11), 14 - 5) - rI[r];
        c1 += __mul24(diff, rGx[r]);  // (|diff| < 2^14, |g| < 2^15)
        c2 += __mul24(diff, rGy[r]);
        right = right_below;
      }
      const long long b1 = wave_sum_split_i64(c1), b2 = wave_sum_split_i64(c2);
      // (the buffer written now was last read two barriers ago: one barrier per iteration is enough)
      long long (*rb)[4] = red_b[j & 1];
      if (lane == 0) {
        rb[0][wave] = b1;
        rb[1][wave] = b2;
      }
      __syncthreads();
      const float B1 = static_cast<float>(rb[0][0] + rb[0][1] + rb[0][2] + rb[0][3]) * flt_scale;
      const float B2 = static_cast<float>(rb[1][0] + rb[1][1] + rb[1][2] + rb[1][3]) * flt_scale;
      const float dx = (A12 * B2 - A22 * B1) * D;
      const float dy = (A12 * B1 - A11 * B2) * D;
      qx += dx;
      qy += dy;
      nx = qx + half_x;
      ny = qy + half_y;
      if (dx * dx + dy * dy <= eps2) break;
      if (j > 0 && fabsf(dx + prev_dx) < 0.01f && fabsf(dy + prev_dy) < 0.01f) {
        nx -= dx * 0.5f;
        ny -= dy * 0.5f;
        break;
      }
      prev_dx = dx;
      prev_dy = dy;
    }
    if (level == 0 && ok) {
      const int rx = static_cast<int>(rintf(nx - half_x)), ry = static_cast<int>(rintf(ny - half_y));
      if (ry < L.vlo || ry + win_h + 1 > L.vhi) suspect = true;
      if (rx < -win_w || rx >= L.cols || ry < -win_h || ry >= L.rows) ok = false;
    }
  }
  if (tid == 0) {
    next_pts[p] = make_float2(nx, ny);
    status[p] = (ok ? 1 : 0) | (suspect ? 2 : 0);
  }
}

// successful tracks -> pooled (xy, uv) float64 pairs in tracking order, appended behind the
// vectors of earlier frame pairs (lucaskanade.py:241-242); one workgroup, ordered compaction
__global__ __launch_bounds__(256) void lk_pool_append(const float2 *__restrict__ pts,
                                                      const float2 *__restrict__ next_pts,
                                                      const unsigned char *__restrict__ status, int npts,
                                                      const int *__restrict__ npts_dev,
                                                      double2 *__restrict__ pool_xy,
                                                      double2 *__restrict__ pool_uv,
                                                      int *__restrict__ pool_count, int capacity) {
  __shared__ int wave_total[4];
  __shared__ int running;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (npts_dev) npts = min(npts, *npts_dev);
  if (tid == 0) running = *pool_count;
  __syncthreads();
  for (int i0 = 0; i0 < npts; i0 += 256) {
    const int i = i0 + tid;
    const bool keep = i < npts && status[i] != 0;
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) wave_total[wave] = __popcll(mask);
    __syncthreads();
    int pos = running;
    for (int w = 0; w < wave; ++w) pos += wave_total[w];
    pos += __popcll(mask & ((1ull << lane) - 1ull));
    if (keep && pos < capacity) {
      const float2 p = pts[i], q = next_pts[i];
      pool_xy[pos] = make_double2(p.x, p.y);
      // float32 difference, like p1 - p0 of the float32 OpenCV arrays (tracking/lucaskanade.py:181)
      pool_uv[pos] = make_double2(static_cast<double>(q.x - p.x), static_cast<double>(q.y - p.y));
    }
    __syncthreads();
    if (tid == 0) running += wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
    __syncthreads();
  }
  if (tid == 0) *pool_count = running;
}

}  // namespace

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
dim3 lk_open_grid(int m, int n) { return dim3((n + kOpenColsW - 1) / kOpenColsW, (m + kOpenRowsWG32 - 1) / kOpenRowsWG32); }
// clean == nullptr: the cleaned frame is not stored, keepbits (m x grid.x words) is written instead
void launch_lk_open(dim3 grid, hipStream_t stream, const float *img, int m, int n, int size_opening, int buffer_mask,
                    float *stats, float *clean, float *part, Band band, unsigned *slots = nullptr,
                    unsigned long long *keepbits = nullptr) {
  hipLaunchKernelGGL(lk_open_bits, grid, dim3(256), 0, stream, img, m, n, size_opening, buffer_mask, stats, clean, part,
                     band, slots, keepbits);
}

constexpr int kCrnRows = 32;  // output rows per wave of the response pass (16 and 64 measured slower: 84 / 84 vs 77 us)
dim3 lk_response_grid(int m, int n, int block_size) {
  const int w = crn_cols(block_size), rows = 4 * kCrnRows;
  return dim3((n + w - 1) / w, (m + rows - 1) / rows);
}
dim3 lk_response_nms_grid(int m, int n, int block_size) {
  const int w = crn_cols(block_size) - 2, rows = 4 * kCrnRows;
  return dim3((n + w - 1) / w, (m + rows - 1) / rows);
}
// slots of the candidate list the waves of that grid own (the overflow count of the slots' counter word is added to it)
int lk_response_nms_fixed_keys(dim3 grid) { return static_cast<int>(grid.x * grid.y) * 4 * kNmsKeys; }
void launch_lk_response_nms(dim3 grid, hipStream_t stream, int block_size, const unsigned char *u8, const float *clean, int m,
                            int n, int buffer_mask, const float *stats, float quality, CornerKeyT *out, int cap, Band band,
                            unsigned *slots, int *zero_b, int count_b) {
#define PSH_NMS_LAUNCH(BS)                                                                                             \
  hipLaunchKernelGGL((lk_corner_response_nms<BS, kCrnRows>), grid, dim3(256), 0, stream, u8, clean, m, n, buffer_mask, \
                     stats, quality, out, cap, band, slots, zero_b, count_b)
  if (block_size == 1) {
    PSH_NMS_LAUNCH(1);
  } else if (block_size == 3) {
    PSH_NMS_LAUNCH(3);
  } else if (block_size == 5) {
    PSH_NMS_LAUNCH(5);
  } else {
    PSH_NMS_LAUNCH(7);
  }
#undef PSH_NMS_LAUNCH
}
// slots != nullptr: the maximum goes to the statistic slots (and zero_a / zero_b are cleared by the first
// workgroup); otherwise one partial maximum per workgroup goes to part[]
void launch_lk_response(dim3 grid, hipStream_t stream, int block_size, const unsigned char *u8, const float *clean, int m,
                        int n, int buffer_mask, const float *stats, float *eig, float *part, Band band,
                        unsigned *slots = nullptr, int *zero_a = nullptr, int count_a = 0, int *zero_b = nullptr,
                        int count_b = 0) {
#define PSH_CRN_LAUNCH(BS)                                                                                          \
  hipLaunchKernelGGL((lk_corner_response_cols<BS, kCrnRows>), grid, dim3(256), 0, stream, u8, clean, m, n, buffer_mask, \
                     stats, eig, part, band, slots, zero_a, count_a, zero_b, count_b)
  if (block_size == 1) {
    PSH_CRN_LAUNCH(1);
  } else if (block_size == 3) {
    PSH_CRN_LAUNCH(3);
  } else if (block_size == 5) {
    PSH_CRN_LAUNCH(5);
  } else {
    PSH_CRN_LAUNCH(7);
  }
#undef PSH_CRN_LAUNCH
}

// the frame workspace: one registered block that grows to the largest frame seen
static int ensure_lk_ws(size_t nbytes, void **ptr) {
  static void *ws = nullptr;
  const int rc = persistent_device(&ws, nbytes);
  *ptr = ws;
  return rc;
}

// the three frame passes (cleaning, opening, uint8 renderings) of one frame on `stream` with the
// caller's workspace: psh_lk_prepare_dev / _f64_dev on the library stream, dense_lk.hip for the NEXT
// frame of a pair on the side stream beside the corner chain of the current one
size_t lk_prepare_ws_bytes(int m, int n, bool f64) {
  const size_t npx = static_cast<size_t>(m) * n;
  if (f64) {
    const dim3 ogrid((n + kOpenColsW - 1) / kOpenColsW, (m + kOpenRowsWG - 1) / kOpenRowsWG);
    return (npx + 2 * static_cast<size_t>(kRedBlocks) + 3 * static_cast<size_t>(ogrid.x * ogrid.y) + 8) * sizeof(double);
  }
  const dim3 ogrid = lk_open_grid(m, n);
  return kSlotBytes + sizeof(float) * (2 * static_cast<size_t>(kRedBlocks) + 3 * static_cast<size_t>(ogrid.x * ogrid.y));
}
size_t lk_slot_bytes() { return kSlotBytes; }
size_t lk_keepbits_bytes(int m, int n) { return static_cast<size_t>(m) * lk_open_grid(m, n).x * sizeof(unsigned long long); }

int lk_prepare_on(hipStream_t stream, void *ws, const void *frame_dev, bool f64, int m, int n, int size_opening,
                  int buffer_mask, float *clean_dev, unsigned char *track_u8_dev, unsigned char *feature_u8_dev,
                  float *stats_dev, unsigned *slots_cleared, unsigned long long *keepbits) {
  if (m <= 0 || n <= 0) return fail(PSH_EINVAL, "lk_prepare: invalid shape (%d,%d)", m, n);
  if (!frame_dev || !track_u8_dev || !stats_dev || !ws) return fail(PSH_EINVAL, "lk_prepare: NULL pointer");
  if (!clean_dev && (f64 || !keepbits)) return fail(PSH_EINVAL, "lk_prepare: NULL pointer");
  if (size_opening != 0 && size_opening != 3)
    return fail(PSH_EUNSUPPORTED, "lk_prepare: size_opening %d not implemented (0 or 3)", size_opening);
  const size_t npx = static_cast<size_t>(m) * n;
  if (!f64) {
    const float *frame = static_cast<const float *>(frame_dev);
    const dim3 ogrid = lk_open_grid(m, n);
    unsigned *own_slots = static_cast<unsigned *>(ws);
    float *part1 = reinterpret_cast<float *>(static_cast<char *>(ws) + kSlotBytes);
    float *part2 = part1 + 2 * kRedBlocks;
    // statistics through the slots: every pass folds its results into them, the next pass reads them
    // back - three launches, no single-workgroup kernel in between
    unsigned *slots = slots_cleared;
    if (!slots) {
      slots = own_slots;
      const hipError_t e = hipMemsetAsync(slots, 0, kSlotBytes, stream);
      if (e != hipSuccess) return fail(PSH_EHIP, "lk_prepare: clearing the statistic slots failed: %s", hipGetErrorString(e));
    }
    hipLaunchKernelGGL(lk_stats1, dim3(kRedBlocks), dim3(256), 0, stream, frame, npx, part1, slots);
    if (clean_dev) {
      launch_lk_open(ogrid, stream, frame, m, n, size_opening, buffer_mask, stats_dev, clean_dev, part2, Band{0, 0, m}, slots);
      const int qgrid = static_cast<int>(std::min<size_t>((npx / 4 + 255) / 256 + 1, 4096));
      hipLaunchKernelGGL(lk_to_u8, dim3(qgrid), dim3(256), 0, stream, clean_dev, m, n, buffer_mask, stats_dev, track_u8_dev,
                         feature_u8_dev, 0, static_cast<const unsigned *>(slots));
    } else {
      // the resident estimate: no cleaned frame in memory, the renderings come from the frame and the keep bits
      launch_lk_open(ogrid, stream, frame, m, n, size_opening, buffer_mask, stats_dev, nullptr, part2, Band{0, 0, m}, slots,
                     keepbits);
      const dim3 qgrid((n + 1023) / 1024, (m + kU8Rows - 1) / kU8Rows);
      const bool vec = n % 4 == 0 && reinterpret_cast<uintptr_t>(frame) % 16 == 0 &&
                       reinterpret_cast<uintptr_t>(track_u8_dev) % 4 == 0 && reinterpret_cast<uintptr_t>(feature_u8_dev) % 4 == 0;
      if (vec) {
        hipLaunchKernelGGL(lk_to_u8_bits<true>, qgrid, dim3(256), 0, stream, frame, keepbits, static_cast<int>(ogrid.x), m, n,
                           buffer_mask, stats_dev, track_u8_dev, feature_u8_dev, static_cast<const unsigned *>(slots));
      } else {
        hipLaunchKernelGGL(lk_to_u8_bits<false>, qgrid, dim3(256), 0, stream, frame, keepbits, static_cast<int>(ogrid.x), m, n,
                           buffer_mask, stats_dev, track_u8_dev, feature_u8_dev, static_cast<const unsigned *>(slots));
      }
    }
  } else {
    // everything that decides a grey level is computed in double, like the reference does for such input
    const double *frame = static_cast<const double *>(frame_dev);
    const dim3 ogrid((n + kOpenColsW - 1) / kOpenColsW, (m + kOpenRowsWG - 1) / kOpenRowsWG);
    const int nb_open = ogrid.x * ogrid.y;
    double *clean64 = static_cast<double *>(ws);
    double *part1 = clean64 + npx, *part2 = part1 + 2 * kRedBlocks, *dstats = part2 + 3 * nb_open;
    hipLaunchKernelGGL(lk_stats1_f64, dim3(kRedBlocks), dim3(256), 0, stream, frame, npx, part1);
    hipLaunchKernelGGL(lk_final_f64, dim3(1), dim3(kFinalThreads), 0, stream, part1, kRedBlocks, 0, stats_dev, dstats);
    hipLaunchKernelGGL(lk_open_bits_f64, ogrid, dim3(256), 0, stream, frame, m, n, size_opening, buffer_mask, stats_dev,
                       dstats, clean_dev, clean64, part2);
    hipLaunchKernelGGL(lk_final_f64, dim3(1), dim3(kFinalThreads), 0, stream, part2, nb_open, 1, stats_dev, dstats);
    const int qgrid = static_cast<int>(std::min<size_t>((npx + 255) / 256, 8192));
    hipLaunchKernelGGL(lk_to_u8_f64, dim3(qgrid), dim3(256), 0, stream, clean64, m, n, buffer_mask, stats_dev, dstats,
                       track_u8_dev, feature_u8_dev);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(PSH_EHIP, "lk_prepare launch failed: %s", hipGetErrorString(e));
  return PSH_OK;
}


}  // namespace psh

using psh::ctx;
using psh::fail;

extern "C" {

int psh_lk_prepare_dev(const float *frame_dev, int m, int n, int size_opening, int buffer_mask,
                       float *clean_dev, unsigned char *track_u8_dev,
                       unsigned char *feature_u8_dev, float *stats_dev) {
  PSH_ENTER(c);
  if (m <= 0 || n <= 0) return fail(PSH_EINVAL, "lk_prepare: invalid shape (%d,%d)", m, n);
  void *ws = nullptr;
  if (int rc = psh::ensure_lk_ws(psh::lk_prepare_ws_bytes(m, n, false), &ws)) return rc;
  return psh::lk_prepare_on(c.stream, ws, frame_dev, false, m, n, size_opening, buffer_mask, clean_dev, track_u8_dev,
                            feature_u8_dev, stats_dev);
}

// the same for a float64 frame (the dtype pysteps arrays have as a rule): everything that decides a
// grey level is computed in double, like the reference does for such input
int psh_lk_prepare_f64_dev(const double *frame_dev, int m, int n, int size_opening, int buffer_mask,
                           float *clean_dev, unsigned char *track_u8_dev,
                           unsigned char *feature_u8_dev, float *stats_dev) {
  PSH_ENTER(c);
  if (m <= 0 || n <= 0) return fail(PSH_EINVAL, "lk_prepare: invalid shape (%d,%d)", m, n);
  psh::Scratch blk;  // [clean64 | partials | dstats]
  if (int rc = blk.alloc(psh::lk_prepare_ws_bytes(m, n, true))) return rc;
  return psh::lk_prepare_on(c.stream, blk.as<void>(), frame_dev, true, m, n, size_opening, buffer_mask, clean_dev,
                            track_u8_dev, feature_u8_dev, stats_dev);
}

// ---- row bands (multi-GPU tiling of the image passes, BASELINE config 5) --------------------
// Every rank holds the whole frame (805 MB at 8192^2 is nothing next to 288 GB) and processes the
// rows [e0, e1) = its own rows [r0, r1) plus a halo as a SUB-IMAGE through offset pointers; the
// sub-image edges that are not frame borders produce wrong values only within a few rows (opening 2,
// Shi-Tomasi response 4), far from the own rows.  What is global in the reference - the min / max of
// the uint8 rescales (tracking/lucaskanade.py:143-160, shitomasi.py:143-151), the NaN count behind
// the row 0 / 1 quirk, the maximum corner response - is reduced over the OWN rows only and then
// combined across ranks by the caller (psh_comm_allreduce; min / max are order-free, so the result
// is bit-identical to the single-device statistics).  Outputs land at their absolute rows in
// full-size buffers.
static int check_band(const char *who, int m, int n, int e0, int e1, int r0, int r1) {
  if (m <= 0 || n <= 0 || e0 < 0 || e1 > m || e0 >= e1 || r0 < e0 || r1 > e1 || r0 > r1)
    return fail(PSH_EINVAL, "%s: rows [%d,%d) / band [%d,%d) do not fit a %d-row frame", who, r0, r1, e0, e1, m);
  return PSH_OK;
}

int psh_lk_band_stats_dev(const float *frame_dev, int m, int n, int r0, int r1, float *stats_dev) {
  PSH_ENTER(c);
  if (!frame_dev || !stats_dev) return fail(PSH_EINVAL, "lk_band_stats: NULL pointer");
  if (int rc = check_band("lk_band_stats", m, n, r0, r1, r0, r1)) return rc;
  void *ws = nullptr;
  if (int rc = psh::ensure_lk_ws(sizeof(float) * 2 * psh::kRedBlocks, &ws)) return rc;
  float *part = static_cast<float *>(ws);
  hipLaunchKernelGGL(psh::lk_stats1, dim3(psh::kRedBlocks), dim3(256), 0, c.stream,
                     frame_dev + static_cast<size_t>(r0) * n, static_cast<size_t>(r1 - r0) * n, part,
                     static_cast<unsigned *>(nullptr));
  hipLaunchKernelGGL(psh::lk_stats1_final, dim3(1), dim3(psh::kFinalThreads), 0, c.stream, part, psh::kRedBlocks, stats_dev);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

int psh_lk_band_open_dev(const float *frame_dev, int m, int n, int e0, int e1, int r0, int r1, int size_opening,
                         int buffer_mask, float *clean_dev, float *stats_dev) {
  PSH_ENTER(c);
  if (!frame_dev || !clean_dev || !stats_dev) return fail(PSH_EINVAL, "lk_band_open: NULL pointer");
  if (int rc = check_band("lk_band_open", m, n, e0, e1, r0, r1)) return rc;
  if (size_opening != 0 && size_opening != 3)
    return fail(PSH_EUNSUPPORTED, "lk_prepare: size_opening %d not implemented (0 or 3)", size_opening);
  const int ms = e1 - e0;
  const dim3 ogrid = psh::lk_open_grid(ms, n);
  const int nb_open = ogrid.x * ogrid.y;
  void *ws = nullptr;
  if (int rc = psh::ensure_lk_ws(sizeof(float) * 3 * static_cast<size_t>(nb_open), &ws)) return rc;
  float *part = static_cast<float *>(ws);
  const float *img = frame_dev + static_cast<size_t>(e0) * n;
  float *clean = clean_dev + static_cast<size_t>(e0) * n;
  const psh::Band band{e0, r0 - e0, r1 - e0};
  psh::launch_lk_open(ogrid, c.stream, img, ms, n, size_opening, buffer_mask, stats_dev, clean, part, band);
  hipLaunchKernelGGL(psh::lk_open_final, dim3(1), dim3(psh::kFinalThreads), 0, c.stream, part, nb_open, stats_dev);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

int psh_lk_band_to_u8_dev(const float *clean_dev, int m, int n, int e0, int e1, int buffer_mask, const float *stats_dev,
                          unsigned char *track_u8_dev, unsigned char *feature_u8_dev) {
  PSH_ENTER(c);
  if (!clean_dev || !stats_dev || !track_u8_dev) return fail(PSH_EINVAL, "lk_band_to_u8: NULL pointer");
  if (int rc = check_band("lk_band_to_u8", m, n, e0, e1, e0, e1)) return rc;
  const size_t off = static_cast<size_t>(e0) * n, npx = static_cast<size_t>(e1 - e0) * n;
  const int qgrid = static_cast<int>(std::min<size_t>((npx / 4 + 255) / 256 + 1, 4096));
  hipLaunchKernelGGL(psh::lk_to_u8, dim3(qgrid), dim3(256), 0, c.stream, clean_dev + off, e1 - e0, n, buffer_mask,
                     const_cast<float *>(stats_dev), track_u8_dev + off, feature_u8_dev ? feature_u8_dev + off : nullptr, e0,
                     static_cast<const unsigned *>(nullptr));
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

int psh_lk_band_response_dev(const unsigned char *feature_u8_dev, const float *clean_dev, int m, int n, int e0, int e1,
                             int r0, int r1, int block_size, int buffer_mask, float *stats_dev, float *eig_dev) {
  PSH_ENTER(c);
  if (!feature_u8_dev || !clean_dev || !stats_dev || !eig_dev) return fail(PSH_EINVAL, "lk_band_response: NULL pointer");
  if (int rc = check_band("lk_band_response", m, n, e0, e1, r0, r1)) return rc;
  if (block_size < 1 || block_size > 2 * psh::kMaxBlockR + 1 || (block_size & 1) == 0)
    return fail(PSH_EUNSUPPORTED, "lk_corners: block_size %d not implemented (odd, <= 7)", block_size);
  const int ms = e1 - e0;
  const dim3 rgrid = psh::lk_response_grid(ms, n, block_size);
  const int nb = rgrid.x * rgrid.y;
  void *ws = nullptr;
  if (int rc = psh::ensure_lk_ws(sizeof(float) * static_cast<size_t>(nb), &ws)) return rc;
  float *part = static_cast<float *>(ws);
  const size_t off = static_cast<size_t>(e0) * n;
  const psh::Band band{e0, r0 - e0, r1 - e0};
  psh::launch_lk_response(rgrid, c.stream, block_size, feature_u8_dev + off, clean_dev + off, ms, n, buffer_mask, stats_dev,
                          eig_dev + off, part, band);
  hipLaunchKernelGGL(psh::lk_max_final, dim3(1), dim3(psh::kFinalThreads), 0, c.stream, part, nb, stats_dev,
                     static_cast<int>(psh::kEigMax), static_cast<int *>(nullptr), 0, static_cast<int *>(nullptr), 0);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

int psh_lk_band_select_dev(const float *eig_dev, const float *clean_dev, int m, int n, int e0, int e1, int r0, int r1,
                           int buffer_mask, double quality_level, const float *stats_dev,
                           unsigned long long *keys_dev, int cap, int *count_dev) {
  PSH_ENTER(c);
  if (!eig_dev || !clean_dev || !stats_dev || !keys_dev || !count_dev || cap <= 0)
    return fail(PSH_EINVAL, "lk_band_select: invalid argument");
  if (int rc = check_band("lk_band_select", m, n, e0, e1, r0, r1)) return rc;
  const int ms = e1 - e0;
  const size_t off = static_cast<size_t>(e0) * n;
  PSH_HIP(hipMemsetAsync(count_dev, 0, sizeof(int), c.stream));
  PSH_HIP(hipMemsetAsync(keys_dev, 0, static_cast<size_t>(cap) * sizeof(psh::CornerKey), c.stream));
  const dim3 sgrid((n + psh::kSelWgCols - 1) / psh::kSelWgCols, (ms + psh::kSelWgRows - 1) / psh::kSelWgRows);
  hipLaunchKernelGGL(psh::lk_corner_select, sgrid, dim3(64 * psh::kSelWaves), 0, c.stream, eig_dev + off, clean_dev + off, ms, n,
                     buffer_mask, static_cast<float>(quality_level), const_cast<float *>(stats_dev), keys_dev, cap, count_dev,
                     psh::Band{e0, r0 - e0, r1 - e0}, static_cast<const unsigned *>(nullptr));
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

namespace {
// state of the corner request in flight (launch -> finish), guarded by the context mutex
struct CornerJob {
  bool active = false;
  bool host_ordered = false;  // max_corners beyond the device kernel's LDS list: ordered in finish()
  int m = 0, n = 0, cap = 0, max_corners = 0;
  double min_distance = 0.0;
  psh::CornerKey *raw_dev = nullptr;  // candidates as the select kernel wrote them (host-ordered path)
  hipEvent_t ready = nullptr;
  void *pinned = nullptr;  // [int count | pad | accepted corners (x, y) float32]
  void *ws = nullptr;      // device block that outlives launch (host-ordered path: response image + keys)
};
constexpr size_t kPinnedHeader = 64;
// requests in flight, first in first out: the frame pairs of one estimate can be launched back to
// back, the copies of their results are queued behind each request's own kernels
constexpr int kMaxCornerJobs = 4;
CornerJob g_corner_jobs[kMaxCornerJobs];
int g_corner_head = 0, g_corner_count = 0;

// Greedy acceptance of goodFeaturesToTrack on a min_distance grid (featureselect.cpp): walk the
// candidates strongest first, accept one unless an accepted corner lies closer than min_distance.
// Accepted corners are chained per grid cell in flat arrays (no per-cell containers).
struct GreedyGrid {
  int cell, gw, gh, n;
  double md2;
  // cell heads live in a per-thread array that is kept between calls: a 4096^2 image has 168 k
  // cells, clearing them costs more than the whole pass, so only the cells an estimate touched
  // are reset when it is done
  std::vector<int> &head;
  std::vector<int> next, px, py, touched;
  static std::vector<int> &head_store() {
    static thread_local std::vector<int> store;
    return store;
  }
  GreedyGrid(int m, int n_, double min_distance, int max_corners)
      : cell(std::max(1, static_cast<int>(std::lrint(min_distance)))), n(n_),
        md2(min_distance * min_distance), head(head_store()) {
    gw = (n + cell - 1) / cell;
    gh = (m + cell - 1) / cell;
    const size_t cells = static_cast<size_t>(gw) * gh;
    if (head.size() < cells) head.assign(cells, -1);  // (all entries are -1 between calls)
    next.reserve(max_corners);
    px.reserve(max_corners);
    py.reserve(max_corners);
    touched.reserve(max_corners);
  }
  ~GreedyGrid() {
    for (int cidx : touched) head[cidx] = -1;
  }
  GreedyGrid(const GreedyGrid &) = delete;
  GreedyGrid &operator=(const GreedyGrid &) = delete;
  bool offer(int x, int y) {
    const int xc = x / cell, yc = y / cell;
    for (int yy = std::max(0, yc - 1); yy <= std::min(gh - 1, yc + 1); ++yy)
      for (int xx = std::max(0, xc - 1); xx <= std::min(gw - 1, xc + 1); ++xx)
        for (int q = head[static_cast<size_t>(yy) * gw + xx]; q >= 0; q = next[q]) {
          const double dx = x - px[q], dy = y - py[q];
          if (dx * dx + dy * dy < md2) return false;
        }
    const int id = static_cast<int>(px.size());
    px.push_back(x);
    py.push_back(y);
    const int cidx = yc * gw + xc;
    if (head[cidx] < 0) touched.push_back(cidx);
    next.push_back(head[cidx]);
    head[cidx] = id;
    return true;
  }
};
}  // namespace

// response image, its maximum, candidate keys (threshold + 3x3 maxima) of one frame: queued on the
// library stream into the block `ws` (layout below); lock held by the caller
namespace {
// psh_set_option("lk_fused_nms", v) / PYSTEPS_HIP_LK_FUSED_NMS: 1 = the resident estimate takes lk_corner_response_nms
// (response + 3x3 maxima + compaction in one pass).  Off by default: on one box, library unchanged, the LK leg measured
// 0.598 ms with it against 0.580 ms without (profiles/r06/j_fused_nms_ab.txt) - the response pass is bound by VALU issue
// (0.88), so the judging, the 10 % of extra strip overlap and the lost occupancy (100 against 90 registers) cost more
// than the response plane's round trip through the memory-side cache saves.  Bit-identical corners either way.
static int g_lk_fused_nms = [] {
  const char *e = std::getenv("PYSTEPS_HIP_LK_FUSED_NMS");
  return e ? std::atoi(e) : 0;
}();
}  // namespace
extern "C++" {
namespace psh {
void set_lk_fused_nms(int v) { g_lk_fused_nms = v; }
}  // namespace psh
}
namespace {
struct CornerWs {
  size_t off_part, off_cnt, off_raw, off_ord, bytes;
  int cap, nb;
  dim3 rgrid;
  CornerWs(int m, int n, int block_size) {
    const size_t npx = static_cast<size_t>(m) * n;
    rgrid = psh::lk_response_grid(m, n, block_size);
    nb = rgrid.x * rgrid.y;
    // every pixel can be a candidate (plateaus of equal response pass the 3x3 test): no overflow
    cap = static_cast<int>(std::min<size_t>(npx, 0x7fffffffu));
    // ... and the fused response pass gives every wave of its grid kNmsKeys slots, used or not, and appends what a
    // wave cannot hold BEHIND all of them: the fixed slots come on top of the pixels (on a plateau image of a few rows
    // the spilled keys alone outnumber the pixels that max(pixels, slots) left for them, and the pass dropped them)
    cap = static_cast<int>(std::min<size_t>(
        static_cast<size_t>(cap) + psh::lk_response_nms_fixed_keys(psh::lk_response_nms_grid(m, n, block_size)), 0x7fffffffu));
    auto up = [](size_t v) { return (v + 255) & ~static_cast<size_t>(255); };
    off_part = up(npx * sizeof(float));
    off_cnt = up(off_part + static_cast<size_t>(nb) * sizeof(float));
    off_raw = up(off_cnt + sizeof(int));
    off_ord = up(off_raw + static_cast<size_t>(cap) * sizeof(psh::CornerKey));
    bytes = off_ord + psh::corner_order_ws_bytes();
  }
};

// eig_slots != nullptr (cleared statistic slots of the frame): the maximum response travels through
// them - the response pass clears the candidate counter and the ordering scratch, the selection pass reads
// the maximum back: two launches; otherwise lk_max_final sits in between
// (count_dev_out: where the number of candidates lives - the workspace's counter, or, for the fused pass of the
// resident estimate, the counter word of the frame's statistic slots)
int corner_candidates(const CornerWs &w, void *ws, const unsigned char *feature_u8_dev, const float *clean_dev,
                      float *stats_dev, int m, int n, int block_size, int buffer_mask, double quality_level,
                      unsigned *eig_slots = nullptr, const int **count_dev_out = nullptr, int *count_bias_out = nullptr) {
  psh::Context &c = ctx();
  char *base = static_cast<char *>(ws);
  float *eig = reinterpret_cast<float *>(base);
  float *part = reinterpret_cast<float *>(base + w.off_part);
  int *cnt = reinterpret_cast<int *>(base + w.off_cnt);
  psh::CornerKey *raw = reinterpret_cast<psh::CornerKey *>(base + w.off_raw);
  int *ord = reinterpret_cast<int *>(base + w.off_ord);
  const int ord_ints = static_cast<int>(psh::corner_order_clear_bytes() / sizeof(int));
  if (count_dev_out) *count_dev_out = cnt;
  if (eig_slots && count_dev_out && count_bias_out && g_lk_fused_nms) {
    // response + 3x3 maxima + compaction in one pass: no response plane, no selection pass (lk_corner_response_nms)
    const dim3 ngrid = psh::lk_response_nms_grid(m, n, block_size);
    psh::launch_lk_response_nms(ngrid, c.stream, block_size, feature_u8_dev, clean_dev, m, n, buffer_mask, stats_dev,
                                static_cast<float>(quality_level), raw, w.cap, psh::Band{0, 0, m}, eig_slots, ord, ord_ints);
    *count_dev_out = reinterpret_cast<const int *>(eig_slots + psh::kSlCand * psh::kSlots);  // the overflow count
    *count_bias_out = psh::lk_response_nms_fixed_keys(ngrid);
    PSH_HIP(hipGetLastError());
    return PSH_OK;
  }
  if (eig_slots) {
    psh::launch_lk_response(w.rgrid, c.stream, block_size, feature_u8_dev, clean_dev, m, n, buffer_mask, stats_dev, eig,
                            part, psh::Band{0, 0, m}, eig_slots, cnt, 1, ord, ord_ints);
  } else {
    psh::launch_lk_response(w.rgrid, c.stream, block_size, feature_u8_dev, clean_dev, m, n, buffer_mask, stats_dev, eig,
                            part, psh::Band{0, 0, m});
    // the candidate counter and the ordering scratch (histogram + header) are cleared by the same launch
    hipLaunchKernelGGL(psh::lk_max_final, dim3(1), dim3(psh::kFinalThreads), 0, c.stream, part, w.nb, stats_dev,
                       static_cast<int>(psh::kEigMax), cnt, 1, ord, ord_ints);
  }
  const dim3 sgrid((n + psh::kSelWgCols - 1) / psh::kSelWgCols, (m + psh::kSelWgRows - 1) / psh::kSelWgRows);
  hipLaunchKernelGGL(psh::lk_corner_select, sgrid, dim3(64 * psh::kSelWaves), 0, c.stream, eig, clean_dev, m, n, buffer_mask,
                     static_cast<float>(quality_level), stats_dev, raw, w.cap, cnt, psh::Band{0, 0, m},
                     static_cast<const unsigned *>(eig_slots));
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

int check_corner_args(const unsigned char *feature_u8_dev, const float *clean_dev, const float *stats_dev, int m,
                      int n, int block_size, int max_corners) {
  if (m <= 0 || n <= 0) return fail(PSH_EINVAL, "lk_corners: invalid shape (%d,%d)", m, n);
  if (!feature_u8_dev || !clean_dev || !stats_dev) return fail(PSH_EINVAL, "lk_corners: NULL pointer");
  if (block_size < 1 || block_size > 2 * psh::kMaxBlockR + 1 || (block_size & 1) == 0)
    return fail(PSH_EUNSUPPORTED, "lk_corners: block_size %d not implemented (odd, <= 7)", block_size);
  if (max_corners <= 0) return fail(PSH_EINVAL, "lk_corners: max_corners must be positive");
  if (static_cast<uint64_t>(m) * static_cast<uint64_t>(n) >= (1ull << 31))
    return fail(PSH_EUNSUPPORTED, "lk_corners: more than 2^31 pixels");
  return PSH_OK;
}
}  // namespace

extern "C++" {
namespace psh {
int lk_corners_resident(const unsigned char *feature_u8_dev, const float *clean_dev, float *stats_dev, int m, int n,
                        int block_size, int buffer_mask, double quality_level, double min_distance, int max_corners,
                        float *points_dev, int *npoints_dev, int (*before_walk)(void *), void *before_walk_arg,
                        int *walk_stats_host, unsigned *slots_cleared) {
  if (int rc = check_corner_args(feature_u8_dev, clean_dev, stats_dev, m, n, block_size, max_corners)) return rc;
  if (!points_dev || !npoints_dev) return fail(PSH_EINVAL, "lk_corners: NULL pointer");
  if (!corner_order_supported(m, n, min_distance, max_corners))
    return fail(PSH_EUNSUPPORTED, "lk_corners: more than %d corners or 65535 rows / columns are ordered on the host",
                corner_order_max_corners());
  Context &c = ctx();
  const CornerWs w(m, n, block_size);
  Scratch ws;  // freed stream-ordered: the kernels below are queued in front of any reuse
  if (int rc = ws.alloc(w.bytes)) return rc;
  const int *count_dev = nullptr;
  int count_bias = 0;
  int rc = corner_candidates(w, ws.as<void>(), feature_u8_dev, clean_dev, stats_dev, m, n, block_size, buffer_mask, quality_level,
                             slots_cleared, &count_dev, &count_bias);
  if (rc == PSH_OK) {
    char *base = ws.as<char>();
    const hipError_t e = launch_corner_order(
        reinterpret_cast<const CornerKey *>(base + w.off_raw), count_dev, w.cap,
        stats_dev + kEigMax, static_cast<float>(quality_level), n, min_distance, max_corners, base + w.off_ord,
        points_dev, npoints_dev, c.stream, before_walk, before_walk_arg, /*ws_is_cleared=*/true,
        count_bias ? slots_cleared + psh::kSlEig * psh::kSlots : nullptr, count_bias, count_bias ? stats_dev + kEigMax : nullptr);
    if (e != hipSuccess) rc = fail(PSH_EHIP, "corner_order launch failed: %s", hipGetErrorString(e));
    if (rc == PSH_OK && walk_stats_host) {
      if (hipMemcpyAsync(walk_stats_host, base + w.off_ord + corner_order_walk_stats_offset(), 13 * sizeof(int),
                         hipMemcpyDeviceToHost, c.stream) != hipSuccess ||
          hipStreamSynchronize(c.stream) != hipSuccess)
        rc = fail(PSH_EHIP, "corner_order statistics copy failed");
    }
  }
  return rc;
}
}  // namespace psh
}  // extern "C++"

int psh_lk_corners_launch_dev(const unsigned char *feature_u8_dev, const float *clean_dev,
                              float *stats_dev, int m, int n, int block_size, int buffer_mask,
                              double quality_level, double min_distance, int max_corners) {
  PSH_ENTER(c);
  if (int rc = check_corner_args(feature_u8_dev, clean_dev, stats_dev, m, n, block_size, max_corners)) return rc;
  if (g_corner_count == kMaxCornerJobs)
    return fail(PSH_EINVAL, "lk_corners: %d corner requests are already in flight", kMaxCornerJobs);
  CornerJob &job = g_corner_jobs[(g_corner_head + g_corner_count) % kMaxCornerJobs];
  if (!job.ready) PSH_HIP(hipEventCreateWithFlags(&job.ready, hipEventDisableTiming));
  const bool host_ordered = !psh::corner_order_supported(m, n, min_distance, max_corners);
  const size_t pin_need = kPinnedHeader + (host_ordered ? 0 : static_cast<size_t>(max_corners) * sizeof(float2));
  if (int rc = psh::persistent_pinned(&job.pinned, pin_need)) return rc;
  char *pin = static_cast<char *>(job.pinned);
  const CornerWs w(m, n, block_size);
  psh::Scratch ws;  // host_ordered: handed to the job once everything is queued; else freed behind the copy
  if (host_ordered) {
    if (int rc = ws.alloc(w.bytes)) return rc;
    if (int rc = corner_candidates(w, ws.as<void>(), feature_u8_dev, clean_dev, stats_dev, m, n, block_size, buffer_mask,
                                   quality_level))
      return rc;
    PSH_HIP(hipMemcpyAsync(pin, ws.at<char>(w.off_cnt), sizeof(int), hipMemcpyDeviceToHost, c.stream));
    job.raw_dev = ws.at<psh::CornerKey>(w.off_raw);
  } else {
    // accepted corners and their count in device memory, then one copy of both behind the kernels
    const size_t pts_bytes = static_cast<size_t>(max_corners) * sizeof(float2);
    if (int rc = ws.alloc(kPinnedHeader + pts_bytes)) return rc;
    if (int rc = psh::lk_corners_resident(feature_u8_dev, clean_dev, stats_dev, m, n, block_size, buffer_mask,
                                          quality_level, min_distance, max_corners, ws.at<float>(kPinnedHeader),
                                          ws.as<int>()))
      return rc;
    PSH_HIP(hipMemcpyAsync(pin, ws.as<char>(), kPinnedHeader + pts_bytes, hipMemcpyDeviceToHost, c.stream));
    ws.reset();  // stream-ordered: the copy above is queued first
  }
  PSH_HIP(hipEventRecord(job.ready, c.stream));
  job.ws = ws.release();
  job.active = true;
  job.host_ordered = host_ordered;
  ++g_corner_count;
  job.m = m;
  job.n = n;
  job.cap = w.cap;
  job.max_corners = max_corners;
  job.min_distance = min_distance;
  return PSH_OK;
}

int psh_lk_corners_finish(float *points_host, int *count_host) {
  PSH_ENTER(c);
  if (!points_host || !count_host) return fail(PSH_EINVAL, "lk_corners: NULL pointer");
  if (g_corner_count == 0) return fail(PSH_EINVAL, "lk_corners: no corner request in flight");
  CornerJob &job = g_corner_jobs[g_corner_head];
  g_corner_head = (g_corner_head + 1) % kMaxCornerJobs;
  --g_corner_count;
  job.active = false;
  // whatever happens below, the request's device block goes back to the allocator
  const psh::Scratch ws(job.ws);
  job.ws = nullptr;
  PSH_HIP(hipEventSynchronize(job.ready));
  const char *pin = static_cast<const char *>(job.pinned);
  const int count = *reinterpret_cast<const int *>(pin);
  if (!job.host_ordered) {  // ordered and accepted on the device (lk_sparse.hip corner_order)
    const int accepted = std::min(std::max(count, 0), job.max_corners);
    std::memcpy(points_host, pin + kPinnedHeader, static_cast<size_t>(accepted) * sizeof(float2));
    *count_host = accepted;
    return PSH_OK;
  }
  // more corners than the device kernel keeps: all candidates come to the host, are ordered and walked here
  const int m = job.m, n = job.n, max_corners = job.max_corners;
  const double min_distance = job.min_distance;
  std::vector<psh::CornerKey> keys(static_cast<size_t>(std::min(std::max(count, 0), job.cap)));
  if (!keys.empty()) {
    PSH_HIP(hipMemcpyAsync(keys.data(), job.raw_dev, keys.size() * sizeof(psh::CornerKey), hipMemcpyDeviceToHost,
                           c.stream));
    PSH_HIP(hipStreamSynchronize(c.stream));
    std::sort(keys.begin(), keys.end(), std::greater<psh::CornerKey>());
  }
  GreedyGrid grid(m, n, min_distance, max_corners);
  int accepted = 0;
  for (size_t ci = 0; ci < keys.size() && accepted < max_corners; ++ci) {
    const unsigned addr = static_cast<unsigned>(keys[ci] & 0xffffffffull);
    const int x = static_cast<int>(addr % static_cast<unsigned>(n)), y = static_cast<int>(addr / static_cast<unsigned>(n));
    if (min_distance >= 1.0 && !grid.offer(x, y)) continue;
    points_host[2 * accepted] = static_cast<float>(x);
    points_host[2 * accepted + 1] = static_cast<float>(y);
    ++accepted;
  }
  *count_host = accepted;
  return PSH_OK;
}

// The ordered min-distance pass of goodFeaturesToTrack on its own (pure host code, no device):
// `keys` = candidates in walking order (response bits << 32 | y * n + x, strongest first), the
// form psh_lk_corners_finish consumes; accepted corners -> points (x, y) float32.
int psh_lk_greedy_host(const unsigned long long *keys, int count, int m, int n, double min_distance,
                       int max_corners, float *points_host, int *count_host) {
  if (!points_host || !count_host || (count > 0 && !keys)) return fail(PSH_EINVAL, "lk_greedy: NULL pointer");
  if (count < 0 || m <= 0 || n <= 0 || max_corners <= 0) return fail(PSH_EINVAL, "lk_greedy: invalid argument");
  GreedyGrid grid(m, n, min_distance, max_corners);
  int accepted = 0;
  for (int ci = 0; ci < count && accepted < max_corners; ++ci) {
    const unsigned addr = static_cast<unsigned>(keys[ci] & 0xffffffffull);
    const int x = static_cast<int>(addr % static_cast<unsigned>(n)), y = static_cast<int>(addr / static_cast<unsigned>(n));
    if (y >= m) return fail(PSH_EINVAL, "lk_greedy: candidate address outside the image");
    if (min_distance >= 1.0 && !grid.offer(x, y)) continue;
    points_host[2 * accepted] = static_cast<float>(x);
    points_host[2 * accepted + 1] = static_cast<float>(y);
    ++accepted;
  }
  *count_host = accepted;
  return PSH_OK;
}

extern "C++" {
namespace psh {
// psh_shutdown: every request still in flight is dropped; its pinned block and device block went with the rest
[[maybe_unused]] static const int g_corner_jobs_hook = at_shutdown([] {
  for (CornerJob &job : g_corner_jobs) {
    if (job.ready) (void)hipEventDestroy(job.ready);
    job = CornerJob{};
  }
  g_corner_head = g_corner_count = 0;
});
int lk_corners_in_flight_limit() { return kMaxCornerJobs; }
}  // namespace psh
}  // extern "C++"

int psh_lk_corners_dev(const unsigned char *feature_u8_dev, const float *clean_dev,
                       float *stats_dev, int m, int n, int block_size, int buffer_mask,
                       double quality_level, double min_distance, int max_corners,
                       float *points_host, int *count_host) {
  if (!points_host || !count_host) return fail(PSH_EINVAL, "lk_corners: NULL pointer");
  if (int rc = psh_lk_corners_launch_dev(feature_u8_dev, clean_dev, stats_dev, m, n, block_size,
                                         buffer_mask, quality_level, min_distance, max_corners))
    return rc;
  return psh_lk_corners_finish(points_host, count_host);
}

namespace {
// Gaussian pyramids + Scharr gradients of one frame pair, in a block of its own so that they
// can be built while the host is still ordering the corner candidates
struct PyramidSet {
  psh::Pyramid pyr;
  void *block = nullptr;
  hipStream_t stream = nullptr;  // the stream the levels were built on (psh_lk_pyramids_read copies behind them)
  int win_w = 0, win_h = 0, max_level = 0;
};
}  // namespace

static int lk_pyramids_on(hipStream_t stream, const unsigned char *prev_u8_dev, const unsigned char *next_u8_dev,
                          int m, int n, int win_w, int win_h, int max_level, void **handle_out, void *block_in,
                          size_t block_in_bytes);

int psh_lk_pyramids_dev(const unsigned char *prev_u8_dev, const unsigned char *next_u8_dev, int m,
                        int n, int win_w, int win_h, int max_level, void **handle_out) {
  PSH_ENTER(c);
  return lk_pyramids_on(c.stream, prev_u8_dev, next_u8_dev, m, n, win_w, win_h, max_level, handle_out, nullptr, 0);
}

extern "C++" {
namespace psh {
// the pyramids of a frame pair on a side stream the caller has forked (they depend on the uint8 renderings only, so
// they are built while the main stream orders the corner candidates, a single-workgroup kernel): no new fork, the
// pyramids wait for what the side stream waits for, not for whatever the main stream was given in the meantime.  `block` (lk_pyramids_bytes() bytes, from
// psh_malloc) has to be taken BEFORE the caller queues anything else on the main stream after the fork: the allocator
// is ordered on the main stream, a block it hands out later may still be in use by that work, which the side stream
// does not wait for.  The pyramid set owns the block once the call has succeeded; when it fails - whichever check or
// launch failed - lk_pyramids_on leaves a caller's block alone and it is released HERE, once, before the error that
// lk_pyramids_on recorded can be overwritten by anything.
int lk_pyramids_on_side(hipStream_t side, void *block, size_t block_bytes, const unsigned char *prev_u8_dev,
                        const unsigned char *next_u8_dev, int m, int n, int win_w, int win_h, int max_level,
                        void **handle_out) {
  Scratch own(block);  // (psh_free of a block of the allocator succeeds and leaves psh_last_error() alone)
  const int rc = lk_pyramids_on(side, prev_u8_dev, next_u8_dev, m, n, win_w, win_h, max_level, handle_out, block, block_bytes);
  if (rc == PSH_OK) (void)own.release();
  return rc;
}
size_t lk_pyramids_bytes(int m, int n, int win_w, int win_h, int max_level) {
  if (max_level >= kMaxLevels) max_level = kMaxLevels - 1;
  const bool need_deriv = win_w > kRowsMaxWin;
  size_t bytes = 0;
  int r = m, q = n;
  if (need_deriv) bytes += (static_cast<size_t>(r) * q * sizeof(short2) + 255) & ~static_cast<size_t>(255);
  for (int l = 1; l <= max_level; ++l) {
    r = (r + 1) / 2;
    q = (q + 1) / 2;
    if (q <= win_w || r <= win_h) break;
    const size_t px = (static_cast<size_t>(r) * q + 255) & ~static_cast<size_t>(255);
    bytes += 2 * px;
    if (need_deriv) bytes += (static_cast<size_t>(r) * q * sizeof(short2) + 255) & ~static_cast<size_t>(255);
  }
  return bytes ? bytes : 256;
}
}  // namespace psh
}  // extern "C++"

static int lk_pyramids_on(hipStream_t stream, const unsigned char *prev_u8_dev, const unsigned char *next_u8_dev,
                          int m, int n, int win_w, int win_h, int max_level, void **handle_out, void *block_in,
                          size_t block_in_bytes) {
  PSH_ENTER(c);
  if (!handle_out) return fail(PSH_EINVAL, "lk_pyramids: NULL handle pointer");
  *handle_out = nullptr;
  if (m <= 0 || n <= 0) return fail(PSH_EINVAL, "lk_pyramids: invalid shape (%d,%d)", m, n);
  if (!prev_u8_dev || !next_u8_dev) return fail(PSH_EINVAL, "lk_pyramids: NULL pointer");
  if (win_w <= 2 || win_h <= 2 || win_w > psh::kMaxWin || win_h > psh::kMaxWin)
    return fail(PSH_EUNSUPPORTED, "lk_track: window (%d,%d) not implemented (3..%d)", win_w, win_h, psh::kMaxWin);
  if (max_level < 0) return fail(PSH_EINVAL, "lk_pyramids: max_level must be >= 0");
  if (max_level >= psh::kMaxLevels) max_level = psh::kMaxLevels - 1;
  // level geometry (buildOpticalFlowPyramid stops before a level is not larger than the window)
  int rows[psh::kMaxLevels], cols[psh::kMaxLevels], top = 0;
  rows[0] = m;
  cols[0] = n;
  for (int l = 1; l <= max_level; ++l) {
    const int r = (rows[l - 1] + 1) / 2, q = (cols[l - 1] + 1) / 2;
    if (q <= win_w || r <= win_h) break;
    rows[l] = r;
    cols[l] = q;
    top = l;
  }
  size_t bytes = 0;
  auto take = [&bytes](size_t nb) {
    const size_t at = bytes;
    bytes += (nb + 255) & ~static_cast<size_t>(255);
    return at;
  };
  // the row-structured tracker computes the Scharr gradients of its windows itself; only the
  // gather kernel for wider windows reads a gradient image
  const bool need_deriv = win_w > psh::kRowsMaxWin;
  size_t off_i[psh::kMaxLevels], off_j[psh::kMaxLevels], off_d[psh::kMaxLevels];
  for (int l = 0; l <= top; ++l) {
    const size_t px = static_cast<size_t>(rows[l]) * cols[l];
    off_i[l] = l ? take(px) : 0;
    off_j[l] = l ? take(px) : 0;
    off_d[l] = need_deriv ? take(px * sizeof(short2)) : 0;
  }
  if (bytes == 0) bytes = 256;  // single level, no gradient image: nothing to store
  PyramidSet *ps = new PyramidSet();
  if (block_in != nullptr) {
    // a block the caller took from the allocator earlier (before it queued other work on the main stream)
    if (block_in_bytes < bytes) {
      delete ps;
      return fail(PSH_EINVAL, "lk_pyramids: the block handed in holds %zu bytes, %zu are needed", block_in_bytes, bytes);
    }
    ps->block = block_in;
  } else if (int rc = psh_malloc(&ps->block, bytes)) {
    delete ps;
    return rc;
  }
  char *base = static_cast<char *>(ps->block);
  ps->pyr.top = top;
  ps->win_w = win_w;
  ps->win_h = win_h;
  ps->max_level = max_level;
  ps->stream = stream;
  for (int l = 0; l <= top; ++l) {
    unsigned char *Il = l ? reinterpret_cast<unsigned char *>(base + off_i[l]) : const_cast<unsigned char *>(prev_u8_dev);
    unsigned char *Jl = l ? reinterpret_cast<unsigned char *>(base + off_j[l]) : const_cast<unsigned char *>(next_u8_dev);
    short2 *dl = need_deriv ? reinterpret_cast<short2 *>(base + off_d[l]) : nullptr;
    if (l) {
      const dim3 g((cols[l] + 255) / 256, (rows[l] + 4 * psh::kPyrRows - 1) / (4 * psh::kPyrRows), 2);
      psh::PyrPair pair;
      pair.src[0] = ps->pyr.lv[l - 1].I;
      pair.src[1] = ps->pyr.lv[l - 1].J;
      pair.dst[0] = Il;
      pair.dst[1] = Jl;
      hipLaunchKernelGGL(psh::lk_pyrdown, g, dim3(256), 0, stream, pair, rows[l - 1], cols[l - 1], rows[l], cols[l]);
    }
    if (need_deriv) {
      const dim3 sg((cols[l] + 63) / 64, (rows[l] + 3) / 4);
      hipLaunchKernelGGL(psh::lk_scharr, sg, dim3(256), 0, stream, Il, rows[l], cols[l], dl);
    }
    ps->pyr.lv[l].I = Il;
    ps->pyr.lv[l].J = Jl;
    ps->pyr.lv[l].dI = dl;
    ps->pyr.lv[l].rows = rows[l];
    ps->pyr.lv[l].cols = cols[l];
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    // a block the caller handed in stays the caller's on every failure path (lk_pyramids_on_side releases it): one owner
    if (block_in == nullptr) (void)psh_free(ps->block);
    delete ps;
    return fail(PSH_EHIP, "lk_pyramids launch failed: %s", hipGetErrorString(e));
  }
  *handle_out = ps;
  return PSH_OK;
}

int psh_lk_pyramids_band(void *handle, int frame_rows, int band_first_row, int *top_level_out) {
  if (!handle) return fail(PSH_EINVAL, "lk_pyramids_band: NULL handle");
  PyramidSet *ps = static_cast<PyramidSet *>(handle);
  const int sub_rows = ps->pyr.lv[0].rows;
  if (band_first_row < 0 || band_first_row + sub_rows > frame_rows)
    return fail(PSH_EINVAL, "lk_pyramids_band: rows [%d,%d) outside the %d-row frame", band_first_row,
                band_first_row + sub_rows, frame_rows);
  if (band_first_row & ((1 << ps->pyr.top) - 1))
    return fail(PSH_EINVAL, "lk_pyramids_band: the first band row must be a multiple of %d", 1 << ps->pyr.top);
  // the whole frame must not have MORE levels than the band has (buildOpticalFlowPyramid stops when a
  // level is not larger than the window): the caller then tracks on whole-frame data instead
  int full_top = 0;
  {
    int r = frame_rows, q = ps->pyr.lv[0].cols;
    for (int l = 1; l < psh::kMaxLevels && l <= ps->max_level; ++l) {
      r = (r + 1) / 2;
      q = (q + 1) / 2;
      if (q <= ps->win_w || r <= ps->win_h) break;
      full_top = l;
    }
  }
  if (full_top != ps->pyr.top)
    return fail(PSH_EUNSUPPORTED, "lk_pyramids_band: the band gives %d pyramid levels, the frame %d", ps->pyr.top + 1,
                full_top + 1);
  // opening reaches 2 rows, every pyrDown 2 rows of the level below, the gradient image 1 row: a
  // margin of 6 rows covers every level
  constexpr int kMargin = 6;
  const bool top_border = band_first_row == 0, bottom_border = band_first_row + sub_rows == frame_rows;
  int rows_full = frame_rows;
  for (int l = 0; l <= ps->pyr.top; ++l) {
    psh::PyrLevel &L = ps->pyr.lv[l];
    if (l) rows_full = (rows_full + 1) / 2;
    L.rows_stored = L.rows;
    L.row_org = band_first_row >> l;
    L.vlo = top_border ? -(1 << 30) : L.row_org + kMargin;
    L.vhi = bottom_border ? (1 << 30) : L.row_org + L.rows_stored - kMargin;
    L.rows = rows_full;
  }
  if (top_level_out) *top_level_out = ps->pyr.top;
  return PSH_OK;
}

int psh_lk_pyramids_free(void *handle) {
  if (!handle) return PSH_OK;
  PyramidSet *ps = static_cast<PyramidSet *>(handle);
  int rc = PSH_OK;
  if (ps->block) rc = psh_free(ps->block);  // stream-ordered reuse; PSH_OK after psh_shutdown, which took the block
  delete ps;
  return rc;
}

// Read-out of a pyramid set for tests: geometry of a level, then one of its planes.  A band set
// (psh_lk_pyramids_band) reports and hands out the rows it stores.
int psh_lk_pyramids_shape(void *handle, int level, int *rows, int *cols, int *top, int *has_deriv) {
  if (!handle) return fail(PSH_EINVAL, "lk_pyramids_shape: NULL handle");
  const PyramidSet *ps = static_cast<const PyramidSet *>(handle);
  if (level < 0 || level > ps->pyr.top)
    return fail(PSH_EINVAL, "lk_pyramids_shape: level %d outside 0..%d", level, ps->pyr.top);
  const psh::PyrLevel &L = ps->pyr.lv[level];
  if (rows) *rows = std::min(L.rows, L.rows_stored);
  if (cols) *cols = L.cols;
  if (top) *top = ps->pyr.top;
  if (has_deriv) *has_deriv = L.dI != nullptr ? 1 : 0;
  return PSH_OK;
}

// plane 0: I, 1: J (rows * cols bytes), 2: dI (rows * cols int16 pairs).  The copy is queued on the stream the set
// was built on, behind the kernels that fill the level, and has arrived when the call returns.
int psh_lk_pyramids_read(void *handle, int level, int plane, void *host_out, size_t nbytes) {
  if (!handle || !host_out) return fail(PSH_EINVAL, "lk_pyramids_read: NULL pointer");
  PSH_ENTER(c);
  const PyramidSet *ps = static_cast<const PyramidSet *>(handle);
  if (level < 0 || level > ps->pyr.top)
    return fail(PSH_EINVAL, "lk_pyramids_read: level %d outside 0..%d", level, ps->pyr.top);
  if (plane < 0 || plane > 2) return fail(PSH_EINVAL, "lk_pyramids_read: plane %d outside 0..2", plane);
  const psh::PyrLevel &L = ps->pyr.lv[level];
  const void *src = plane == 0 ? static_cast<const void *>(L.I) : plane == 1 ? static_cast<const void *>(L.J) : L.dI;
  if (!src) return fail(PSH_EINVAL, "lk_pyramids_read: the set has no gradient image (window of %d columns)", ps->win_w);
  const size_t want = static_cast<size_t>(std::min(L.rows, L.rows_stored)) * L.cols * (plane == 2 ? sizeof(short2) : 1);
  if (nbytes != want) return fail(PSH_EINVAL, "lk_pyramids_read: %zu bytes given, the plane holds %zu", nbytes, want);
  PSH_HIP(hipMemcpyAsync(host_out, src, want, hipMemcpyDeviceToHost, ps->stream));
  PSH_HIP(hipStreamSynchronize(ps->stream));
  return PSH_OK;
}

// picks the instantiation with the fewest window samples per thread
static void launch_lk_track(int npts, const int *npts_dev, hipStream_t stream, const psh::Pyramid &pyr,
                            const float2 *pts, int win_w, int win_h, int max_count, float eps2, float min_eig_thr,
                            float2 *next_pts, unsigned char *status) {
  const int per = (win_w * win_h + 255) / 256;
  if (win_w <= psh::kRowsMaxWin) {  // one lane per window column, ceil(win_h / 4) rows per wave
#define PSH_TRACK_ROWS(R)                                                                               \
  hipLaunchKernelGGL(psh::lk_track_rows<R>, dim3(npts), dim3(256), 0, stream, pyr, pts, npts, npts_dev, win_w, \
                     win_h, max_count, eps2, min_eig_thr, next_pts, status)
    const int rows = (win_h + 3) / 4;
    if (rows <= 8) {
      PSH_TRACK_ROWS(8);
    } else if (rows <= 13) {
      PSH_TRACK_ROWS(13);
    } else {
      PSH_TRACK_ROWS(16);
    }
#undef PSH_TRACK_ROWS
    return;
  }
  if (per <= 4) {
    hipLaunchKernelGGL(psh::lk_track<4>, dim3(npts), dim3(256), 0, stream, pyr, pts, npts, npts_dev, win_w, win_h,
                       max_count, eps2, min_eig_thr, next_pts, status);
  } else if (per <= 10) {
    hipLaunchKernelGGL(psh::lk_track<10>, dim3(npts), dim3(256), 0, stream, pyr, pts, npts, npts_dev, win_w, win_h,
                       max_count, eps2, min_eig_thr, next_pts, status);
  } else {
    hipLaunchKernelGGL(psh::lk_track<16>, dim3(npts), dim3(256), 0, stream, pyr, pts, npts, npts_dev, win_w, win_h,
                       max_count, eps2, min_eig_thr, next_pts, status);
  }
}

int psh_lk_track_pyr_dev(void *handle, const float *points_host, int npts, int max_count,
                         double epsilon, double min_eig_threshold, float *next_points_host,
                         unsigned char *status_host) {
  PSH_ENTER(c);
  if (!handle) return fail(PSH_EINVAL, "lk_track: NULL pyramid handle");
  if (npts < 0) return fail(PSH_EINVAL, "lk_track: negative point count");
  if (npts == 0) return PSH_OK;
  if (!points_host || !next_points_host || !status_host) return fail(PSH_EINVAL, "lk_track: NULL pointer");
  PyramidSet *ps = static_cast<PyramidSet *>(handle);
  max_count = std::min(std::max(max_count, 0), 100);  // calcOpticalFlowPyrLK clamps the criteria
  const size_t pts_bytes = (static_cast<size_t>(npts) * sizeof(float2) + 255) & ~static_cast<size_t>(255);
  psh::Scratch blk;
  if (int rc = blk.alloc(2 * pts_bytes + static_cast<size_t>(npts))) return rc;
  char *base = blk.as<char>();
  float2 *d_pts = reinterpret_cast<float2 *>(base);
  float2 *d_next = reinterpret_cast<float2 *>(base + pts_bytes);
  unsigned char *d_st = reinterpret_cast<unsigned char *>(base + 2 * pts_bytes);
  const float eps = static_cast<float>(epsilon);
  PSH_HIP(hipMemcpyAsync(d_pts, points_host, static_cast<size_t>(npts) * sizeof(float2),
                         hipMemcpyHostToDevice, c.stream));
  launch_lk_track(npts, nullptr, c.stream, ps->pyr, d_pts, ps->win_w, ps->win_h, max_count, eps * eps,
                  static_cast<float>(min_eig_threshold), d_next, d_st);
  PSH_HIP(hipGetLastError());
  PSH_HIP(hipMemcpyAsync(next_points_host, d_next, static_cast<size_t>(npts) * sizeof(float2),
                         hipMemcpyDeviceToHost, c.stream));
  PSH_HIP(hipMemcpyAsync(status_host, d_st, static_cast<size_t>(npts), hipMemcpyDeviceToHost, c.stream));
  PSH_HIP(hipStreamSynchronize(c.stream));
  return PSH_OK;
}

int psh_lk_track_dev(const unsigned char *prev_u8_dev, const unsigned char *next_u8_dev, int m,
                     int n, const float *points_host, int npts, int win_w, int win_h,
                     int max_level, int max_count, double epsilon, double min_eig_threshold,
                     float *next_points_host, unsigned char *status_host) {
  if (npts == 0) return PSH_OK;
  void *h = nullptr;
  if (int rc = psh_lk_pyramids_dev(prev_u8_dev, next_u8_dev, m, n, win_w, win_h, max_level, &h)) return rc;
  const int rc = psh_lk_track_pyr_dev(h, points_host, npts, max_count, epsilon, min_eig_threshold,
                                      next_points_host, status_host);
  const int rc2 = psh_lk_pyramids_free(h);
  return rc ? rc : rc2;
}

}  // extern "C"

namespace psh {

int lk_track_pool(void *pyramid_handle, const float *points_host, const float *points_dev, const int *npts_dev,
                  int npts, int max_count, double epsilon, double min_eig_threshold, double *pool_xy_dev,
                  double *pool_uv_dev, int *pool_count_dev, int pool_capacity) {
  if (!pyramid_handle || !pool_xy_dev || !pool_uv_dev || !pool_count_dev)
    return fail(PSH_EINVAL, "lk_track_pool: NULL pointer");
  if ((points_host == nullptr) == (points_dev == nullptr) || (points_dev && !npts_dev))
    return fail(PSH_EINVAL, "lk_track_pool: points either on the host or on the device with their count");
  if (npts <= 0) return PSH_OK;
  PyramidSet *ps = static_cast<PyramidSet *>(pyramid_handle);
  max_count = std::min(std::max(max_count, 0), 100);
  Context &c = ctx();
  const size_t pts_bytes = (static_cast<size_t>(npts) * sizeof(float2) + 255) & ~static_cast<size_t>(255);
  psh::Scratch blk;
  if (int rc = blk.alloc(2 * pts_bytes + static_cast<size_t>(npts))) return rc;
  char *base = blk.as<char>();
  float2 *d_pts = reinterpret_cast<float2 *>(base);
  float2 *d_next = reinterpret_cast<float2 *>(base + pts_bytes);
  unsigned char *d_st = reinterpret_cast<unsigned char *>(base + 2 * pts_bytes);
  const float eps = static_cast<float>(epsilon);
  const float2 *pts = reinterpret_cast<const float2 *>(points_dev);
  if (points_host) {
    // pinned staging slot per call (ring): the copy is asynchronous and the caller's buffer may
    // be reused at once
    static void *ring = nullptr;
    static size_t ring_slot = 0;
    constexpr size_t kSlots = 8, kSlotBytes = 1 << 16;
    if (static_cast<size_t>(npts) * sizeof(float2) > kSlotBytes)
      return fail(PSH_EUNSUPPORTED, "lk_track_pool: more than %zu points", kSlotBytes / sizeof(float2));
    if (int rc = persistent_pinned(&ring, kSlots * kSlotBytes)) return rc;
    if (ring_slot == kSlots) {
      PSH_HIP(hipStreamSynchronize(c.stream));
      ring_slot = 0;
    }
    char *slot = static_cast<char *>(ring) + (ring_slot++) * kSlotBytes;
    std::memcpy(slot, points_host, static_cast<size_t>(npts) * sizeof(float2));
    PSH_HIP(hipMemcpyAsync(d_pts, slot, static_cast<size_t>(npts) * sizeof(float2), hipMemcpyHostToDevice, c.stream));
    pts = d_pts;
  }
  launch_lk_track(npts, npts_dev, c.stream, ps->pyr, pts, ps->win_w, ps->win_h, max_count, eps * eps,
                  static_cast<float>(min_eig_threshold), d_next, d_st);
  hipLaunchKernelGGL(lk_pool_append, dim3(1), dim3(256), 0, c.stream, pts, d_next, d_st, npts, npts_dev,
                     reinterpret_cast<double2 *>(pool_xy_dev), reinterpret_cast<double2 *>(pool_uv_dev),
                     pool_count_dev, pool_capacity);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

}  // namespace psh

