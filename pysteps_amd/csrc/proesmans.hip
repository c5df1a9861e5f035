// The Proesmans motion estimate (pysteps/motion/proesmans.py, _proesmans.pyx; Proesmans et al. 1994) on gfx950.
//
// Everything is float64 and uses the reference's operations in the reference's order, without contraction to fused
// multiply-adds (the pragma below), with IEEE division and square root: given the same K the device's planes equal
// the reference's bit for bit.  The one thing not reproduced is the raster-order running sum c_sum behind
// K = 0.9 c_sum / c_count: here it is a double-double sum in a fixed order, rounded once.
//
// The sweep.  The reference updates V in place in raster order: pixel (y, x) reads (y-1, x-1), (y-1, x), (y-1, x+1) and
// (y, x-1) after this sweep wrote them and (y, x+1), (y+1, x-1), (y+1, x), (y+1, x+1) before.  In t = x + 2 y the new
// values lie at t-3 .. t-1 and the old ones at t+1 .. t+3, so all pixels of one t are independent.  A wave owns
// kSweepRows consecutive rows, one lane per row, and steps through t: lane r handles x = t - 2 r.  Its left neighbour
// and the three values of the row above stay in registers; the row above hands over one new value per step by a lane
// shift.  Lane 0 reads the row above from memory: that row belongs to the wave above, which an earlier launch has
// taken past those pixels.  A wave runs kSweepSteps steps, a tile (rb, tb) of the (row block, t block) plane with t
// counted from the block's first row; kSweepSteps = 2 kSweepRows makes tile (rb, tb) depend on (rb-1, tb+1),
// (rb-1, tb) and (rb, tb-1) alone, and its old values of block rb+1 lie in tiles (rb+1, tb-1) and (rb+1, tb).  One
// launch takes the tiles with 2 rb + tb = d, both directions: what a tile needs has run in launches d-1 and d-2, what
// must not have run yet comes in d+1 and d+2.  No workgroup waits for another.
#include <algorithm>

#include "common.h"
#include "dd.h"

#pragma clang fp contract(off)

namespace psh {
namespace {

constexpr int kThreads = 256;
constexpr int kSweepRows = 64;                 // one wave: a lane per row
constexpr int kSweepSteps = 2 * kSweepRows;    // t per tile (see above: the dependency pattern relies on the factor 2)
constexpr int kMaxPartials = 1024;             // blocks of a reduction's first stage
constexpr double kIntensityScale = 1.0 / 255.0;

void *g_ws = nullptr;        // whole call: pyramids, gradients, GAMMA, two V
void *g_reduce = nullptr;    // partial sums of the first reduction stage and their results

struct ReduceBlock {
  dd sum[2][kMaxPartials];
  long long count[2][kMaxPartials];
  double lo[kMaxPartials], hi[kMaxPartials], bad[kMaxPartials];
  double stats[2][4];   // per direction {c_sum, c_count, K, 0}
  double range[4];      // {min, max, non-finite count, 0}
};

__device__ __forceinline__ double at(const double *I, int h, int w, int y, int x) {
  return (y >= 0 && y < h && x >= 0 && x < w) ? I[static_cast<size_t>(y) * w + x] : 0.0;
}

// _linear_interpolate: truncation toward zero, indices clamped, weights from the clamped indices
__device__ __forceinline__ double interpolate(const double *I, int h, int w, double x, double y) {
  int x0 = static_cast<int>(x), y0 = static_cast<int>(y);
  int x1 = x0 + 1, y1 = y0 + 1;
  x0 = min(max(x0, 0), w - 1);
  x1 = min(max(x1, 0), w - 1);
  y0 = min(max(y0, 0), h - 1);
  y1 = min(max(y1, 0), h - 1);
  const double Ia = I[static_cast<size_t>(y0) * w + x0], Ib = I[static_cast<size_t>(y1) * w + x0];
  const double Ic = I[static_cast<size_t>(y0) * w + x1], Id = I[static_cast<size_t>(y1) * w + x1];
  const double wa = (x1 - x) * (y1 - y), wb = (x1 - x) * (y - y0);
  const double wc = (x - x0) * (y1 - y), wd = (x - x0) * (y - y0);
  return wa * Ia + wb * Ib + wc * Ic + wd * Id;
}

// ---- 1. normalisation ------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kThreads) void range_partial(const T *__restrict__ in, size_t count, ReduceBlock *rb) {
  __shared__ double s_lo[kThreads], s_hi[kThreads], s_bad[kThreads];
  double lo = INFINITY, hi = -INFINITY, bad = 0.0;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < count; i += static_cast<size_t>(gridDim.x) * kThreads) {
    const double v = static_cast<double>(in[i]);
    if (isfinite(v)) {
      lo = fmin(lo, v);
      hi = fmax(hi, v);
    } else {
      bad += 1.0;
    }
  }
  s_lo[threadIdx.x] = lo, s_hi[threadIdx.x] = hi, s_bad[threadIdx.x] = bad;
  __syncthreads();
  for (int d = kThreads / 2; d >= 1; d >>= 1) {
    if (static_cast<int>(threadIdx.x) < d) {
      s_lo[threadIdx.x] = fmin(s_lo[threadIdx.x], s_lo[threadIdx.x + d]);
      s_hi[threadIdx.x] = fmax(s_hi[threadIdx.x], s_hi[threadIdx.x + d]);
      s_bad[threadIdx.x] += s_bad[threadIdx.x + d];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) rb->lo[blockIdx.x] = s_lo[0], rb->hi[blockIdx.x] = s_hi[0], rb->bad[blockIdx.x] = s_bad[0];
}

__global__ __launch_bounds__(kThreads) void range_finish(ReduceBlock *rb, int nparts) {
  __shared__ double s_lo[kThreads], s_hi[kThreads], s_bad[kThreads];
  double lo = INFINITY, hi = -INFINITY, bad = 0.0;
  for (int i = threadIdx.x; i < nparts; i += kThreads) {
    lo = fmin(lo, rb->lo[i]);
    hi = fmax(hi, rb->hi[i]);
    bad += rb->bad[i];  // whole numbers below 2^53: exact in any order
  }
  s_lo[threadIdx.x] = lo, s_hi[threadIdx.x] = hi, s_bad[threadIdx.x] = bad;
  __syncthreads();
  for (int d = kThreads / 2; d >= 1; d >>= 1) {
    if (static_cast<int>(threadIdx.x) < d) {
      s_lo[threadIdx.x] = fmin(s_lo[threadIdx.x], s_lo[threadIdx.x + d]);
      s_hi[threadIdx.x] = fmax(s_hi[threadIdx.x], s_hi[threadIdx.x + d]);
      s_bad[threadIdx.x] += s_bad[threadIdx.x + d];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) rb->range[0] = s_lo[0], rb->range[1] = s_hi[0], rb->range[2] = s_bad[0], rb->range[3] = 0.0;
}

// (im - min) / (max - min) * 255.0 when max - min > 1e-8, else the values as they are
template <typename T>
__global__ __launch_bounds__(kThreads) void scale_frames(const T *__restrict__ in, size_t count, const ReduceBlock *rb,
                                                         double *__restrict__ out) {
  const double lo = rb->range[0], hi = rb->range[1];
  const double span = hi - lo;
  for (size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; i < count; i += static_cast<size_t>(gridDim.x) * kThreads) {
    const double v = static_cast<double>(in[i]);
    out[i] = span > 1e-8 ? (v - lo) / span * 255.0 : v;
  }
}

// ---- 2. pyramid ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void pyramid_level(const double *__restrict__ src, int n, int dh, int dw,
                                                          double *__restrict__ dst) {
  const int x = blockIdx.x * kThreads + threadIdx.x, y = blockIdx.y;
  if (x >= dw || y >= dh) return;
  const double *p = src + static_cast<size_t>(2 * y) * n + 2 * x;
  dst[static_cast<size_t>(y) * dw + x] = (p[0] + p[1] + p[n] + p[n + 1]) / 4.0;
}

// ---- 3. gradients ----------------------------------------------------------------------------------------------
// scipy.ndimage.convolve(I, K, mode="constant", cval=0.0): the kernel flipped, a sum that starts at 0.0 and takes the
// non-zero taps in raster order of the flipped kernel; a tap outside the image adds weight * 0.0
__global__ __launch_bounds__(kThreads) void gradients(const double *__restrict__ I, int m, int n, double *__restrict__ G) {
  const int x = blockIdx.x * kThreads + threadIdx.x, y = blockIdx.y;
  if (x >= n || y >= m) return;
  const double w1 = 1.0 / 8.0 * kIntensityScale, w2 = 2.0 / 8.0 * kIntensityScale;
  const double a = at(I, m, n, y - 1, x - 1), b = at(I, m, n, y - 1, x), c = at(I, m, n, y - 1, x + 1);
  const double d = at(I, m, n, y, x - 1), e = at(I, m, n, y, x + 1);
  const double f = at(I, m, n, y + 1, x - 1), g = at(I, m, n, y + 1, x), h = at(I, m, n, y + 1, x + 1);
  double gx = 0.0;
  gx = gx + -w1 * a;
  gx = gx + w1 * c;
  gx = gx + -w2 * d;
  gx = gx + w2 * e;
  gx = gx + -w1 * f;
  gx = gx + w1 * h;
  double gy = 0.0;
  gy = gy + -w1 * a;
  gy = gy + -w2 * b;
  gy = gy + -w1 * c;
  gy = gy + w1 * f;
  gy = gy + w2 * g;
  gy = gy + w1 * h;
  const size_t plane = static_cast<size_t>(m) * n, i = static_cast<size_t>(y) * n + x;
  G[i] = gx;
  G[plane + i] = gy;
}

// ---- 4. consistency maps ---------------------------------------------------------------------------------------
// raw c of both directions (blockIdx.y) into GAMMA, -1 where the displaced pixel leaves the image; the block's
// double-double sum and count of the c it wrote go to the reduction block
__global__ __launch_bounds__(kThreads) void consistency_raw(const double *__restrict__ V, int m, int n, double *__restrict__ GAMMA,
                                                            ReduceBlock *rb) {
  __shared__ dd s_sum[kThreads / 64];
  __shared__ long long s_cnt[kThreads / 64];
  const int i = blockIdx.y;
  const size_t plane = static_cast<size_t>(m) * n;
  const double *V11 = V + (2 * i) * plane, *V12 = V11 + plane;
  const double *V21 = V + (2 * (1 - i)) * plane, *V22 = V21 + plane;
  double *out = GAMMA + i * plane;
  dd sum = {0.0, 0.0};
  long long cnt = 0;
  for (size_t p = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; p < plane; p += static_cast<size_t>(gridDim.x) * kThreads) {
    const int y = static_cast<int>(p / n), x = static_cast<int>(p - static_cast<size_t>(y) * n);
    const double u = V11[p], v = V12[p];
    const double xd = x + u, yd = y + v;
    double c = -1.0;
    if (xd >= 0 && yd >= 0 && xd < n && yd < m) {
      const double uDiff = u + interpolate(V21, m, n, xd, yd);
      const double vDiff = v + interpolate(V22, m, n, xd, yd);
      c = sqrt(uDiff * uDiff + vDiff * vDiff);
      sum = dd_add_d(sum, c);
      ++cnt;
    }
    out[p] = c;
  }
  sum = dd_wave_sum(sum);
  for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d);
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = sum, s_cnt[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kThreads / 64; ++w) sum = dd_add(sum, s_sum[w]), cnt += s_cnt[w];
    rb->sum[i][blockIdx.x] = sum;
    rb->count[i][blockIdx.x] = cnt;
  }
}

// one block per direction: the partial sums in a fixed order, rounded once; K = 0.9 c_sum / c_count
__global__ __launch_bounds__(kThreads) void consistency_finish(ReduceBlock *rb, int nparts) {
  __shared__ dd s_sum[kThreads / 64];
  __shared__ long long s_cnt[kThreads / 64];
  const int i = blockIdx.x;
  dd sum = {0.0, 0.0};
  long long cnt = 0;
  for (int p = threadIdx.x; p < nparts; p += kThreads) sum = dd_add(sum, rb->sum[i][p]), cnt += rb->count[i][p];
  sum = dd_wave_sum(sum);
  for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d);
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = sum, s_cnt[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kThreads / 64; ++w) sum = dd_add(sum, s_sum[w]), cnt += s_cnt[w];
    const double c_sum = sum.hi + sum.lo;
    const double K = cnt > 0 ? 0.9 * c_sum / static_cast<double>(cnt) : 0.0;
    rb->stats[i][0] = c_sum, rb->stats[i][1] = static_cast<double>(cnt), rb->stats[i][2] = K, rb->stats[i][3] = 0.0;
  }
}

__global__ __launch_bounds__(kThreads) void consistency_normalise(double *__restrict__ GAMMA, size_t plane, const ReduceBlock *rb) {
  const int i = blockIdx.y;
  const double K = rb->stats[i][2];
  double *g = GAMMA + i * plane;
  for (size_t p = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x; p < plane; p += static_cast<size_t>(gridDim.x) * kThreads) {
    double out = 1.0;
    if (K > 1e-8) {
      const double c = g[p];
      if (c >= 0.0) out = 1.0 / (1.0 + (c / K) * (c / K));
    }
    g[p] = out;
  }
}

// ---- 5. the sweep ----------------------------------------------------------------------------------------------
struct SweepArgs {
  const double *R;      // (2, m, n) frames of this level
  const double *G;      // (2, 2, m, n): [frame][gx, gy]
  const double *GAMMA;  // (2, m, n)
  double *V;            // (2, 2, m, n), updated in place
  int m, n;
  double lam;
};

// tile (rb_first + blockIdx.x, d - 2 rb) of direction blockIdx.y; one wave
__global__ __launch_bounds__(kSweepRows) void sweep_tiles(SweepArgs a, int d, int rb_first) {
  const int m = a.m, n = a.n;
  const int j = blockIdx.y;
  const int rb = rb_first + blockIdx.x, tb = d - 2 * rb;
  const int r = threadIdx.x;
  const int y = rb * kSweepRows + r;
  const size_t plane = static_cast<size_t>(m) * n;
  const double *gam = a.GAMMA + j * plane;
  double *V0 = a.V + (2 * j) * plane, *V1 = V0 + plane;
  const double *R1 = a.R + j * plane, *R2 = a.R + (1 - j) * plane;
  const double *Gx = a.G + (2 * j) * plane, *Gy = Gx + plane;
  const bool row_ok = y >= 1 && y <= m - 2;
  int x = tb * kSweepSteps - 2 * r;  // this lane's pixel at the tile's first step
  // values of step -1 and before: all final, written by earlier launches (or edge values, which a sweep leaves alone)
  double mine0 = at(V0, m, n, y, x - 1), mine1 = at(V1, m, n, y, x - 1);
  double up0 = at(V0, m, n, y - 1, x), up1 = at(V1, m, n, y - 1, x);
  double ul0 = at(V0, m, n, y - 1, x - 1), ul1 = at(V1, m, n, y - 1, x - 1);
  // What a step reads without needing the step before it slides through registers and is loaded one step ahead, so
  // that the only load a step waits for is the sample of the other frame: GAMMA's columns x-1, x, x+1 (rows y-1, y,
  // y+1), the old V of row y+1 at x-1, x, x+1 and of row y at x and x+1, the frame and its gradients at (y, x), and
  // lane 0's (y-1, x+1).  The old values are not overwritten before step t+1, so an earlier read sees the same.
  double gl[3], gm[3], gr[3];
  for (int k = 0; k < 3; ++k) {
    gl[k] = at(gam, m, n, y - 1 + k, x - 1), gm[k] = at(gam, m, n, y - 1 + k, x), gr[k] = at(gam, m, n, y - 1 + k, x + 1);
  }
  double dl0 = at(V0, m, n, y + 1, x - 1), d0 = at(V0, m, n, y + 1, x), dr0 = at(V0, m, n, y + 1, x + 1);
  double dl1 = at(V1, m, n, y + 1, x - 1), d1 = at(V1, m, n, y + 1, x), dr1 = at(V1, m, n, y + 1, x + 1);
  double here0 = at(V0, m, n, y, x), here1 = at(V1, m, n, y, x);
  double rt0 = at(V0, m, n, y, x + 1), rt1 = at(V1, m, n, y, x + 1);
  double r1 = at(R1, m, n, y, x), gx = at(Gx, m, n, y, x), gy = at(Gy, m, n, y, x);
  double top0 = r == 0 ? at(V0, m, n, y - 1, x + 1) : 0.0, top1 = r == 0 ? at(V1, m, n, y - 1, x + 1) : 0.0;
  for (int s = 0; s < kSweepSteps; ++s, ++x) {
    // the next step's values
    const double ng0 = at(gam, m, n, y - 1, x + 2), ng1 = at(gam, m, n, y, x + 2), ng2 = at(gam, m, n, y + 1, x + 2);
    const double ndr0 = at(V0, m, n, y + 1, x + 2), ndr1 = at(V1, m, n, y + 1, x + 2);
    const double nrt0 = at(V0, m, n, y, x + 2), nrt1 = at(V1, m, n, y, x + 2);
    const double nr1 = at(R1, m, n, y, x + 1), ngx = at(Gx, m, n, y, x + 1), ngy = at(Gy, m, n, y, x + 1);
    // lane 0's row above lies in the block above; its tile of these t ran in an earlier launch, the one after it may
    // be running now and is not looked at
    const bool more = r == 0 && s + 1 < kSweepSteps;
    const double ntop0 = more ? at(V0, m, n, y - 1, x + 2) : 0.0, ntop1 = more ? at(V1, m, n, y - 1, x + 2) : 0.0;
    // (y-1, x+1): what the lane above produced one step ago
    double ur0 = __shfl_up(mine0, 1), ur1 = __shfl_up(mine1, 1);
    if (r == 0) ur0 = top0, ur1 = top1;
    double new0 = here0, new1 = here1;  // not an interior pixel: the value a sweep leaves alone
    if (row_ok && x >= 1 && x <= n - 2) {
      const size_t c = static_cast<size_t>(y) * n + x;
      const double g_u = gm[0], g_l = gl[1], g_r = gr[1], g_d = gm[2];
      const double g_ul = gl[0], g_ur = gr[0], g_dl = gl[2], g_dr = gr[2];
      const double sw = (g_u + g_l + g_r + g_d) / 6.0 + (g_ul + g_ur + g_dl + g_dr) / 12.0;
      double avg0 = 0.0, avg1 = 0.0;
      if (sw > 1e-8) {
        const double s0 = (g_u * up0 + g_l * mine0 + g_r * rt0 + g_d * d0) / 6.0 +
                          (g_ul * ul0 + g_ur * ur0 + g_dl * dl0 + g_dr * dr0) / 12.0;
        const double s1 = (g_u * up1 + g_l * mine1 + g_r * rt1 + g_d * d1) / 6.0 +
                          (g_ul * ul1 + g_ur * ur1 + g_dl * dl1 + g_dr * dr1) / 12.0;
        avg0 = s0 / sw;
        avg1 = s1 / sw;
      }
      const double xd = x + avg0, yd = y + avg1;
      new0 = avg0, new1 = avg1;
      if (xd >= 0 && xd < n - 1 && yd >= 0 && yd < m - 1) {
        const double It = (interpolate(R2, m, n, xd, yd) - r1) * kIntensityScale;
        const double ic = a.lam * It / (1.0 + a.lam * (gx * gx + gy * gy));
        new0 = avg0 - gx * ic;
        new1 = avg1 - gy * ic;
      }
      V0[c] = new0;
      V1[c] = new1;
    }
    ul0 = up0, ul1 = up1;
    up0 = ur0, up1 = ur1;
    mine0 = new0, mine1 = new1;
    for (int k = 0; k < 3; ++k) gl[k] = gm[k], gm[k] = gr[k];
    gr[0] = ng0, gr[1] = ng1, gr[2] = ng2;
    dl0 = d0, d0 = dr0, dr0 = ndr0;
    dl1 = d1, d1 = dr1, dr1 = ndr1;
    here0 = rt0, here1 = rt1;
    rt0 = nrt0, rt1 = nrt1;
    r1 = nr1, gx = ngx, gy = ngy;
    top0 = ntop0, top1 = ntop1;
  }
}

// _fill_edges of the four planes (blockIdx.y): edges from the first / last interior row or column, corners from the
// diagonal interior pixel; reads interior pixels only
__global__ __launch_bounds__(kThreads) void fill_edges(double *__restrict__ V, int m, int n) {
  double *P = V + static_cast<size_t>(blockIdx.y) * m * n;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= 1 && i <= n - 2) {
    P[i] = P[static_cast<size_t>(n) + i];
    P[static_cast<size_t>(m - 1) * n + i] = P[static_cast<size_t>(m - 2) * n + i];
  }
  if (i >= 1 && i <= m - 2) {
    P[static_cast<size_t>(i) * n] = P[static_cast<size_t>(i) * n + 1];
    P[static_cast<size_t>(i) * n + n - 1] = P[static_cast<size_t>(i) * n + n - 2];
  }
  if (i == 0) {
    P[0] = P[static_cast<size_t>(n) + 1];
    P[n - 1] = P[static_cast<size_t>(n) + n - 2];
    P[static_cast<size_t>(m - 1) * n] = P[static_cast<size_t>(m - 2) * n + 1];
    P[static_cast<size_t>(m - 1) * n + n - 1] = P[static_cast<size_t>(m - 2) * n + n - 2];
  }
}

// ---- 6. next level ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void next_level(const double *__restrict__ Vp, int mp, int np, double *__restrict__ Vn, int mn,
                                                       int nn) {
  const int xn = blockIdx.x * kThreads + threadIdx.x, yn = blockIdx.y;
  if (xn >= nn || yn >= mn) return;
  const size_t pp = static_cast<size_t>(mp) * np, pn = static_cast<size_t>(mn) * nn;
  const size_t o = static_cast<size_t>(yn) * nn + xn;
  if (xn % 2 != 0 || yn % 2 != 0) {
    const double xc = xn / 2.0, yc = yn / 2.0;
    for (int k = 0; k < 4; ++k) Vn[k * pn + o] = 2.0 * interpolate(Vp + k * pp, mp, np, xc, yc);
  } else {
    const int xci = min(xn / 2, np - 1), yci = min(yn / 2, mp - 1);
    for (int k = 0; k < 4; ++k) Vn[k * pn + o] = 2.0 * Vp[k * pp + static_cast<size_t>(yci) * np + xci];
  }
}

// ---- host side -------------------------------------------------------------------------------------------------
int blocks_1d(size_t count) { return static_cast<int>(std::min<size_t>(kMaxPartials, (count + kThreads - 1) / kThreads)); }
dim3 grid_2d(int m, int n) { return dim3((n + kThreads - 1) / kThreads, m); }

int check_shape(const char *what, int m, int n) {
  if (m < 3 || n < 3) return fail(PSH_EINVAL, "%s: shape %d x %d (each side at least 3)", what, m, n);
  if (static_cast<long long>(m) * n > (1LL << 28) || m > 65535) return fail(PSH_EUNSUPPORTED, "%s: shape %d x %d too large", what, m, n);
  return PSH_OK;
}

int reduce_block(ReduceBlock **rb) {
  if (int rc = persistent_device(&g_reduce, sizeof(ReduceBlock))) return rc;
  *rb = static_cast<ReduceBlock *>(g_reduce);
  return PSH_OK;
}

int sweep_tile_columns(int n) { return (n + 2 * (kSweepRows - 1) - 2) / kSweepSteps + 1; }  // t = x + 2 r up to n - 2 + 2 * 63
int sweep_row_blocks(int m) { return (m - 2) / kSweepRows + 1; }                            // rows 1 .. m - 2

int consistency_on(hipStream_t stream, const double *V, int m, int n, double *GAMMA, ReduceBlock *rb) {
  const size_t plane = static_cast<size_t>(m) * n;
  const int nb = blocks_1d(plane);
  hipLaunchKernelGGL(consistency_raw, dim3(nb, 2), dim3(kThreads), 0, stream, V, m, n, GAMMA, rb);
  PSH_HIP(hipGetLastError());
  hipLaunchKernelGGL(consistency_finish, dim3(2), dim3(kThreads), 0, stream, rb, nb);
  PSH_HIP(hipGetLastError());
  hipLaunchKernelGGL(consistency_normalise, dim3(nb, 2), dim3(kThreads), 0, stream, GAMMA, plane, static_cast<const ReduceBlock *>(rb));
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

int sweep_on(hipStream_t stream, const SweepArgs &a) {
  const int n_rb = sweep_row_blocks(a.m), n_tb = sweep_tile_columns(a.n);
  for (int d = 0; d <= 2 * (n_rb - 1) + n_tb - 1; ++d) {
    const int first = std::max(0, (d - (n_tb - 1) + 1) / 2), last = std::min(n_rb - 1, d / 2);
    if (last < first) continue;
    hipLaunchKernelGGL(sweep_tiles, dim3(last - first + 1, 2), dim3(kSweepRows), 0, stream, a, d, first);
    PSH_HIP(hipGetLastError());
  }
  const int side = std::max(a.m, a.n);
  hipLaunchKernelGGL(fill_edges, dim3((side + kThreads - 1) / kThreads, 4), dim3(kThreads), 0, stream, a.V, a.m, a.n);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

}  // namespace
}  // namespace psh

extern "C" int psh_proesmans_sweep_launches(int m, int n) {
  using namespace psh;
  if (m < 3 || n < 3) return 0;
  const int n_rb = sweep_row_blocks(m), n_tb = sweep_tile_columns(n);
  int launches = 1;  // the edge fill
  for (int d = 0; d <= 2 * (n_rb - 1) + n_tb - 1; ++d)
    if (std::min(n_rb - 1, d / 2) >= std::max(0, (d - (n_tb - 1) + 1) / 2)) ++launches;
  return launches;
}

extern "C" int psh_proesmans_scale_dev(const void *frames_dev, int f32, size_t count, double *out_dev, double *range_host) {
  using namespace psh;
  PSH_ENTER(c);
  if (!frames_dev || !out_dev || !range_host) return fail(PSH_EINVAL, "proesmans_scale: NULL pointer");
  if (count < 1) return fail(PSH_EINVAL, "proesmans_scale: no values");
  ReduceBlock *rb = nullptr;
  if (int rc = reduce_block(&rb)) return rc;
  const int nb = blocks_1d(count);
  if (int rc = with_real(frames_dev, !f32, [&](auto *in) -> int {
        hipLaunchKernelGGL(range_partial, dim3(nb), dim3(kThreads), 0, c.stream, in, count, rb);
        PSH_HIP(hipGetLastError());
        hipLaunchKernelGGL(range_finish, dim3(1), dim3(kThreads), 0, c.stream, rb, nb);
        PSH_HIP(hipGetLastError());
        hipLaunchKernelGGL(scale_frames, dim3(nb), dim3(kThreads), 0, c.stream, in, count, static_cast<const ReduceBlock *>(rb), out_dev);
        PSH_HIP(hipGetLastError());
        return PSH_OK;
      }))
    return rc;
  PSH_HIP(hipMemcpyAsync(range_host, rb->range, 3 * sizeof(double), hipMemcpyDeviceToHost, c.stream));
  PSH_HIP(hipStreamSynchronize(c.stream));
  return PSH_OK;
}

extern "C" int psh_proesmans_pyramid_dev(const double *src_dev, int m, int n, double *dst_dev) {
  using namespace psh;
  PSH_ENTER(c);
  if (!src_dev || !dst_dev) return fail(PSH_EINVAL, "proesmans_pyramid: NULL pointer");
  if (m < 2 || n < 2 || m / 2 > 65535) return fail(PSH_EINVAL, "proesmans_pyramid: shape %d x %d", m, n);
  hipLaunchKernelGGL(pyramid_level, grid_2d(m / 2, n / 2), dim3(kThreads), 0, c.stream, src_dev, n, m / 2, n / 2, dst_dev);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

extern "C" int psh_proesmans_gradients_dev(const double *frame_dev, int m, int n, double *grad_dev) {
  using namespace psh;
  PSH_ENTER(c);
  if (!frame_dev || !grad_dev) return fail(PSH_EINVAL, "proesmans_gradients: NULL pointer");
  if (m < 1 || n < 1 || m > 65535) return fail(PSH_EINVAL, "proesmans_gradients: shape %d x %d", m, n);
  hipLaunchKernelGGL(gradients, grid_2d(m, n), dim3(kThreads), 0, c.stream, frame_dev, m, n, grad_dev);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

extern "C" int psh_proesmans_consistency_dev(const double *V_dev, int m, int n, double *gamma_dev, double *raw_dev, double *stats_dev) {
  using namespace psh;
  PSH_ENTER(c);
  if (!V_dev || !gamma_dev) return fail(PSH_EINVAL, "proesmans_consistency: NULL pointer");
  if (int rc = check_shape("proesmans_consistency", m, n)) return rc;
  ReduceBlock *rb = nullptr;
  if (int rc = reduce_block(&rb)) return rc;
  const size_t plane = static_cast<size_t>(m) * n;
  const int nb = blocks_1d(plane);
  hipLaunchKernelGGL(consistency_raw, dim3(nb, 2), dim3(kThreads), 0, c.stream, V_dev, m, n, gamma_dev, rb);
  PSH_HIP(hipGetLastError());
  if (raw_dev) PSH_HIP(hipMemcpyAsync(raw_dev, gamma_dev, 2 * plane * sizeof(double), hipMemcpyDeviceToDevice, c.stream));
  hipLaunchKernelGGL(consistency_finish, dim3(2), dim3(kThreads), 0, c.stream, rb, nb);
  PSH_HIP(hipGetLastError());
  hipLaunchKernelGGL(consistency_normalise, dim3(nb, 2), dim3(kThreads), 0, c.stream, gamma_dev, plane, static_cast<const ReduceBlock *>(rb));
  PSH_HIP(hipGetLastError());
  if (stats_dev) PSH_HIP(hipMemcpyAsync(stats_dev, rb->stats, 8 * sizeof(double), hipMemcpyDeviceToDevice, c.stream));
  return PSH_OK;
}

extern "C" int psh_proesmans_sweep_dev(const double *frames_dev, const double *grad_dev, const double *gamma_dev, double *V_dev, int m,
                                       int n, double lam) {
  using namespace psh;
  PSH_ENTER(c);
  if (!frames_dev || !grad_dev || !gamma_dev || !V_dev) return fail(PSH_EINVAL, "proesmans_sweep: NULL pointer");
  if (int rc = check_shape("proesmans_sweep", m, n)) return rc;
  return sweep_on(c.stream, SweepArgs{frames_dev, grad_dev, gamma_dev, V_dev, m, n, lam});
}

extern "C" int psh_proesmans_next_level_dev(const double *V_prev_dev, int m_prev, int n_prev, double *V_next_dev, int m_next, int n_next) {
  using namespace psh;
  PSH_ENTER(c);
  if (!V_prev_dev || !V_next_dev) return fail(PSH_EINVAL, "proesmans_next_level: NULL pointer");
  if (m_prev < 1 || n_prev < 1 || m_next < 1 || n_next < 1 || m_next > 65535)
    return fail(PSH_EINVAL, "proesmans_next_level: %d x %d -> %d x %d", m_prev, n_prev, m_next, n_next);
  if (m_next / 2 > m_prev || n_next / 2 > n_prev)
    return fail(PSH_EINVAL, "proesmans_next_level: %d x %d is not the level above %d x %d", m_next, n_next, m_prev, n_prev);
  hipLaunchKernelGGL(next_level, grid_2d(m_next, n_next), dim3(kThreads), 0, c.stream, V_prev_dev, m_prev, n_prev, V_next_dev, m_next,
                     n_next);
  PSH_HIP(hipGetLastError());
  return PSH_OK;
}

extern "C" int psh_proesmans_dev(const double *frames_dev, int m, int n, double lam, int num_iter, int num_levels, int f32,
                                 void *V_dev, void *gamma_dev) {
  using namespace psh;
  PSH_ENTER(c);
  if (!frames_dev || !V_dev || !gamma_dev) return fail(PSH_EINVAL, "proesmans: NULL pointer");
  if (num_levels < 1 || num_levels > 30 || num_iter < 0) return fail(PSH_EINVAL, "proesmans: num_levels %d, num_iter %d", num_levels, num_iter);
  if (int rc = check_shape("proesmans", m, n)) return rc;
  int lm[32], ln[32];
  lm[0] = m, ln[0] = n;
  for (int l = 1; l < num_levels; ++l) lm[l] = lm[l - 1] / 2, ln[l] = ln[l - 1] / 2;
  if (lm[num_levels - 1] < 3 || ln[num_levels - 1] < 3)
    return fail(PSH_EUNSUPPORTED, "proesmans: coarsest level %d x %d (each side at least 3)", lm[num_levels - 1], ln[num_levels - 1]);
  ReduceBlock *rb = nullptr;
  if (int rc = reduce_block(&rb)) return rc;
  // workspace (doubles): levels 1.. of both frames as (2, m_l, n_l) stacks, G (2, 2, m, n), GAMMA (2, m, n), two V (2, 2, m, n)
  const size_t plane = static_cast<size_t>(m) * n;
  size_t pyr = 0;
  for (int l = 1; l < num_levels; ++l) pyr += 2 * static_cast<size_t>(lm[l]) * ln[l];
  if (int rc = persistent_device(&g_ws, (pyr + 14 * plane) * sizeof(double))) return rc;
  double *ws = static_cast<double *>(g_ws);
  const double *R[32];
  R[0] = frames_dev;
  double *next = ws;
  for (int l = 1; l < num_levels; ++l) {
    const size_t pl = static_cast<size_t>(lm[l]) * ln[l], pprev = static_cast<size_t>(lm[l - 1]) * ln[l - 1];
    for (int f = 0; f < 2; ++f) {
      hipLaunchKernelGGL(pyramid_level, grid_2d(lm[l], ln[l]), dim3(kThreads), 0, c.stream, R[l - 1] + f * pprev, ln[l - 1], lm[l], ln[l],
                         next + f * pl);
      PSH_HIP(hipGetLastError());
    }
    R[l] = next;
    next += 2 * pl;
  }
  double *G = next, *GAMMA = G + 4 * plane, *Vcur = GAMMA + 2 * plane, *Vnext = Vcur + 4 * plane;
  const int top = num_levels - 1;
  PSH_HIP(hipMemsetAsync(Vcur, 0, 4 * static_cast<size_t>(lm[top]) * ln[top] * sizeof(double), c.stream));
  for (int l = top; l >= 0; --l) {
    const size_t pl = static_cast<size_t>(lm[l]) * ln[l];
    for (int f = 0; f < 2; ++f) {
      hipLaunchKernelGGL(gradients, grid_2d(lm[l], ln[l]), dim3(kThreads), 0, c.stream, R[l] + f * pl, lm[l], ln[l], G + 2 * f * pl);
      PSH_HIP(hipGetLastError());
    }
    const SweepArgs a{R[l], G, GAMMA, Vcur, lm[l], ln[l], lam};
    for (int it = 0; it < num_iter; ++it) {
      if (int rc = consistency_on(c.stream, Vcur, lm[l], ln[l], GAMMA, rb)) return rc;
      if (int rc = sweep_on(c.stream, a)) return rc;
    }
    if (l > 0) {
      hipLaunchKernelGGL(next_level, grid_2d(lm[l - 1], ln[l - 1]), dim3(kThreads), 0, c.stream, static_cast<const double *>(Vcur), lm[l],
                         ln[l], Vnext, lm[l - 1], ln[l - 1]);
      PSH_HIP(hipGetLastError());
      std::swap(Vcur, Vnext);
    }
  }
  if (int rc = consistency_on(c.stream, Vcur, m, n, GAMMA, rb)) return rc;
  if (f32) {
    PSH_HIP(launch_convert_f64_f32(Vcur, static_cast<float *>(V_dev), 4 * plane, c.stream));
    PSH_HIP(launch_convert_f64_f32(GAMMA, static_cast<float *>(gamma_dev), 2 * plane, c.stream));
  } else {
    PSH_HIP(hipMemcpyAsync(V_dev, Vcur, 4 * plane * sizeof(double), hipMemcpyDeviceToDevice, c.stream));
    PSH_HIP(hipMemcpyAsync(gamma_dev, GAMMA, 2 * plane * sizeof(double), hipMemcpyDeviceToDevice, c.stream));
  }
  return PSH_OK;
}
