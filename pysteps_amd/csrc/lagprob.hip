// The Lagrangian probability nowcast (pysteps/nowcasts/lagrangian_probability.py, Germann and Zawadzki 2004) on
// gfx950: the probability stage behind the extrapolator.
//
// The reference convolves two 0/1 maps of the advected field (exceed = field >= threshold, valid = not NaN) with a
// 0/1 disc (a square below scale 5) and divides them.  Every output is therefore the quotient of two small integers;
// the kernels here count them instead of convolving:
//   lagprob_prefix  per row the exclusive prefix counts of both maps, packed as two 16-bit halves of one uint32
//                   (exceed low, valid high), rows of n + 1 words with a leading zero (the scan of row_prefix.h).  Both prefixes are monotone, so
//                   a difference of two packed words never borrows, and a disc of diameter <= 255 sums to < 65536
//                   per half.
//   lagprob_count   a workgroup owns a 64 x 16 output tile and walks the scale + 15 prefix rows it needs in chunks of
//                   32 rows staged in LDS.  Columns are clamped to [0, n] and rows outside the image are zero while
//                   staging, so the inner loop is one packed difference per kernel row, without a border branch:
//                   scale LDS differences per pixel instead of scale^2 taps.  The row spans of the flipped and centred
//                   kernel come from the host (pysteps_amd/nowcasts/lagrangian_probability.py kernel_spans) and ride
//                   in the kernel arguments.  One float64 divide, NaN where the advected field is NaN.
// Integer throughout, no atomics, no data-dependent loops: the result is deterministic and equals the correctly rounded
// quotient of the two counts.
#include "common.h"
#include "row_prefix.h"

namespace psh {
namespace {

constexpr int kLagMaxScale = 255;
constexpr int kLagMaxWidth = kPackedPrefixMaxWidth;  // a packed row prefix has 16 bits per map
constexpr int kLagThreads = 256;
constexpr int kLagTileW = 64;   // output columns of a workgroup = lanes of a wave
constexpr int kLagRowsPerWave = 4;
constexpr int kLagTileH = 4 * kLagRowsPerWave;  // 4 waves
constexpr int kLagChunk = 32;   // prefix rows staged at a time
constexpr int kLagMaxStage = kLagTileW + kLagMaxScale + 1;  // staged words per row

// ab[t] = a | b << 16: staged columns (relative to the pixel's lane) of the left and right end of kernel row t
struct LagSpans {
  uint32_t ab[kLagMaxScale + 1];
};

template <typename T>
__global__ __launch_bounds__(kLagThreads) void lagprob_prefix(const T *__restrict__ field, int n, double threshold,
                                                               uint32_t *__restrict__ prefix) {
  __shared__ uint32_t wave_sum[kLagThreads / 64];
  const size_t row = blockIdx.x;
  const T *src = field + row * n;
  packed_row_prefix<kLagThreads>(n, prefix + row * (static_cast<size_t>(n) + 1), wave_sum, [&](int x) {
    const T f = src[x];
    const bool valid = !(f != f);
    const bool exceed = valid && static_cast<double>(f) >= threshold;
    return (exceed ? 1u : 0u) | (valid ? 0x10000u : 0u);
  });
}

template <typename T>
__global__ __launch_bounds__(kLagThreads) void lagprob_count(const T *__restrict__ field, const uint32_t *__restrict__ prefix,
                                                              int m, int n, int scale, LagSpans spans,
                                                              double *__restrict__ out) {
  __shared__ uint32_t stage[kLagChunk * kLagMaxStage];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = (scale - 1) / 2;
  const int width = kLagTileW + scale + 1;            // staged words per row
  const int x0 = blockIdx.x * kLagTileW, y0 = blockIdx.y * kLagTileH;
  const int col0 = x0 - (scale - c);                  // prefix column of staged word 0
  const int row0 = y0 + c - scale + 1;                // image row of halo row 0
  const int halo = kLagTileH + scale - 1;
  const size_t pitch = static_cast<size_t>(n) + 1;
  const int ly0 = wave * kLagRowsPerWave;             // first tile row of this wave

  uint32_t acc[kLagRowsPerWave];
#pragma unroll
  for (int k = 0; k < kLagRowsPerWave; ++k) acc[k] = 0u;

  for (int h0 = 0; h0 < halo; h0 += kLagChunk) {
    const int rows = min(kLagChunk, halo - h0);
    __syncthreads();
    for (int r = wave; r < rows; r += kLagThreads / 64) {
      const int g = row0 + h0 + r;
      const bool inside = g >= 0 && g < m;
      const uint32_t *src = prefix + (inside ? g : 0) * pitch;
      for (int j = lane; j < width; j += 64) {
        const int col = min(max(col0 + j, 0), n);
        stage[r * width + j] = inside ? src[col] : 0u;
      }
    }
    __syncthreads();
    // halo rows ly .. ly + scale - 1 belong to tile row ly; kernel row t = halo row - ly
    const int first = max(0, ly0 - h0), last = min(rows, ly0 + kLagRowsPerWave - 1 + scale - h0);
    for (int r = first; r < last; ++r) {
      const uint32_t *line = stage + r * width + lane;
#pragma unroll
      for (int k = 0; k < kLagRowsPerWave; ++k) {
        const int t = h0 + r - (ly0 + k);
        if (t >= 0 && t < scale) {
          const uint32_t ab = spans.ab[t];
          PSH_DASSERT((ab & 0xffffu) <= (ab >> 16) && lane + static_cast<int>(ab >> 16) < width);
          acc[k] += line[ab >> 16] - line[ab & 0xffffu];
        }
      }
    }
  }

  const int x = x0 + lane;
  if (x >= n) return;
#pragma unroll
  for (int k = 0; k < kLagRowsPerWave; ++k) {
    const int y = y0 + ly0 + k;
    if (y >= m) break;
    const size_t at = static_cast<size_t>(y) * n + x;
    const T f = field[at];
    const double exceed = static_cast<double>(acc[k] & 0xffffu), valid = static_cast<double>(acc[k] >> 16);
    out[at] = (f != f) ? static_cast<double>(NAN) : exceed / valid;
  }
}

template <typename T>
int run_planes(const T *fields, int T_planes, int m, int n, double threshold, const int *scales, const int *lo, const int *hi,
               uint32_t *prefix, double *out, hipStream_t s) {
  const size_t plane = static_cast<size_t>(m) * n;
  const dim3 grid((n + kLagTileW - 1) / kLagTileW, (m + kLagTileH - 1) / kLagTileH);
  int at = 0;
  for (int i = 0; i < T_planes; ++i) {
    const int scale = scales[i], c = (scale - 1) / 2;
    LagSpans spans = {};
    for (int t = 0; t < scale; ++t) {
      // pixel x sums prefix[x + hi + 1] - prefix[x + lo]; the staged row starts at column x0 - (scale - c)
      const int a = lo[at + t] + scale - c, b = hi[at + t] + 1 + scale - c;
      if (a < 0 || b < a || b > scale + 1)
        return fail(PSH_EINVAL, "lagprob: span [%d, %d] of kernel row %d does not fit scale %d", lo[at + t], hi[at + t], t, scale);
      spans.ab[t] = static_cast<uint32_t>(a) | (static_cast<uint32_t>(b) << 16);
    }
    at += scale;
    const T *field = fields + i * plane;
    hipLaunchKernelGGL(lagprob_prefix<T>, dim3(m), dim3(kLagThreads), 0, s, field, n, threshold, prefix);
    PSH_HIP(hipGetLastError());
    hipLaunchKernelGGL(lagprob_count<T>, grid, dim3(kLagThreads), 0, s, field, static_cast<const uint32_t *>(prefix), m, n, scale,
                       spans, out + i * plane);
    PSH_HIP(hipGetLastError());
  }
  return PSH_OK;
}

}  // namespace
}  // namespace psh

using psh::fail;

extern "C" int psh_lagprob_dev(const void *fields_dev, int fields_f64, int T, int m, int n, double threshold,
                               const int *scales_host, const int *span_lo_host, const int *span_hi_host, double *out_dev) {
  using namespace psh;
  PSH_ENTER(c);
  if (m < 1 || n < 1) return fail(PSH_EINVAL, "lagprob: invalid shape (%d,%d)", m, n);
  if (n > kLagMaxWidth) return fail(PSH_EUNSUPPORTED, "lagprob: width %d (1..%d)", n, kLagMaxWidth);
  if (T < 1 || T > 65536) return fail(PSH_EINVAL, "lagprob: %d planes", T);
  if (!fields_dev || !scales_host || !span_lo_host || !span_hi_host || !out_dev) return fail(PSH_EINVAL, "lagprob: NULL pointer");
  for (int i = 0; i < T; ++i)
    if (scales_host[i] < 1 || scales_host[i] > kLagMaxScale)
      return fail(PSH_EUNSUPPORTED, "lagprob: scale %d (1..%d)", scales_host[i], kLagMaxScale);
  psh::Scratch blk;
  if (int rc = blk.alloc(static_cast<size_t>(m) * (static_cast<size_t>(n) + 1) * sizeof(uint32_t))) return rc;
  uint32_t *prefix = blk.as<uint32_t>();
  return with_real(fields_dev, fields_f64 != 0, [&](auto *fields) {
    return run_planes(fields, T, m, n, threshold, scales_host, span_lo_host, span_hi_host, prefix, out_dev, c.stream);
  });
}
