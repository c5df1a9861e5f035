/* Aggregation, clipping and squaring of resident fields: the part of the C ABI of libpysteps_hip.so that
 * csrc/dimension.hip implements.  Included by pysteps_hip.h (status codes and conventions are described there); not
 * meant to be included alone. */
#ifndef PYSTEPS_HIP_DIMENSION_H
#define PYSTEPS_HIP_DIMENSION_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- aggregation, clipping and squaring of resident fields (csrc/dimension.hip) ----------------------------------- *
 * pysteps/utils/dimension.py.  float32 and float64 (is_f64), any element alignment (16-byte vectors where the addresses
 * allow, the same arithmetic element by element elsewhere); every call is queued on the library stream.  A window is
 * added strictly in index order starting from +0, in the field's own type - what NumPy does when it reduces a
 * non-innermost axis - so results carry the reference's bits (a window of -0.0 gives +0.0).  PSH_AGG_NANSUM / NANMEAN add +0 for a NaN;
 * MEAN / NANMEAN divide by the window size / the count of non-NaN entries (the float64 quotient stored in the field's
 * type, as NumPy forms it); a window of NaN only gives 0 / NaN.
 *  psh_aggregate_axis_dev   a C-contiguous array seen as (pre, len, post) -> (pre, len / window, post).  trim != 0: the
 *      last len % window entries of the axis are not read; otherwise window has to divide len.
 *  psh_aggregate_space_dev  (planes, m, n) -> (planes, m / wy, n / wx), the upscale of aggregate_fields_space: the mean
 *      (ignore_nan: nanmean) over wy rows, rounded in the field's type, then over wx of those.  PSH_SPACE_AUTO: one fused
 *      kernel for windows up to PSH_SPACE_MAX_WINDOW in both directions, else two psh_aggregate_axis_dev passes through
 *      a scratch plane; PSH_SPACE_FUSED / PSH_SPACE_TWO_LAUNCH force a route (same bits either way).
 *  psh_accumulate_step_dev  the running form of an aggregation along time: first != 0 stores 0 + the input (n
 *      elements) in acc_dev, else adds it; float32 input may meet a float64 accumulator (widened exactly).  count_dev (n uint32,
 *      PSH_AGG_NANMEAN only; otherwise unused and may be NULL) counts the non-NaN inputs.  last != 0: MEAN divides by
 *      nframes, NANMEAN by the count, in the same launch.
 *  psh_window_copy_dev      out (planes, out_m, out_n) = fill, except the h x w rectangle at (dst_y, dst_x), which
 *      receives the rectangle at (src_y, src_x) of in (planes, in_m, in_n); values and fill are converted to the output
 *      type (clip_domain, square_domain and their inverses; float32 -> float64 is the widening `np.ones() * value` implies)
 *  psh_field_min_dev        np.min of n elements: NaN if any element is NaN, an infinity is a value.  Waits for the
 *      library stream */
#define PSH_AGG_SUM 0
#define PSH_AGG_MEAN 1
#define PSH_AGG_NANSUM 2
#define PSH_AGG_NANMEAN 3
#define PSH_SPACE_AUTO 0
#define PSH_SPACE_FUSED 1
#define PSH_SPACE_TWO_LAUNCH 2
#define PSH_SPACE_MAX_WINDOW 64
int psh_aggregate_axis_dev(const void *in_dev, int is_f64, size_t pre, size_t len, size_t post, int window, int method,
                           int trim, void *out_dev);
int psh_aggregate_space_dev(const void *in_dev, int is_f64, size_t planes, int m, int n, int wy, int wx, int ignore_nan,
                            int route, void *out_dev);
int psh_accumulate_step_dev(const void *in_dev, int in_f64, void *acc_dev, int acc_f64, unsigned *count_dev, size_t n,
                            int method, int first, int last, int nframes);
int psh_window_copy_dev(const void *in_dev, int in_f64, size_t planes, int in_m, int in_n, int src_y, int src_x,
                        void *out_dev, int out_f64, int out_m, int out_n, int dst_y, int dst_x, int h, int w, double fill);
int psh_field_min_dev(const void *in_dev, int is_f64, size_t n, double *min_out);

#ifdef __cplusplus
}
#endif
#endif /* PYSTEPS_HIP_DIMENSION_H */
