"""Temporal autocorrelation of a time series of fields on the GPU (mirror of pysteps/timeseries/correlation.py,
``temporal_autocorrelation``) - what every STEPS-family nowcast runs per cascade level before its main loop
(nowcasts/steps.py:838-843, sprog.py:289-297, sseps.py:445, blending/steps.py:1491, pca_ens_kalman_filter.py:445, and
anvil.py in the moving-window form).

The reference takes one ``np.corrcoef`` per cascade level and lag: two boolean-indexed copies of the planes, their
centring and a BLAS product.  Here one launch reads a whole cascade ``(L, T, ...)`` once and returns, per level and
lag, the sums a correlation coefficient is made of, as double-double pairs with exact products
(``psh_autocorr_sums_dev``, csrc/autocorr.hip).  The host forms

    (S_ab - S_a S_b / N) / sqrt((S_aa - S_a^2 / N) (S_bb - S_b^2 / N))

from them in exact rational arithmetic and rounds once, so a coefficient is the correctly rounded one of the sums
(which carry ~106 bits), whatever cancels.  A variance below 2^-96 of the plane's mean square is below what the sums
resolve and counts as zero: a constant plane gives NaN like the reference.

* ``domain="spectral"``: the sums of pysteps/utils/spectral.py ``corrcoef`` over the spectra
  (``psh_autocorr_spectral_sums_dev``); the DC terms are subtracted on the host as the reference writes them.
* ``window_radius < inf``: the six Gaussian-filtered planes of ``_moving_window_corrcoef`` from ``psh_anvil_gauss_dev``
  (bit-identical with SciPy) and the element-wise finish in the reference's operation order
  (``psh_window_corrcoef_dev``): the planes equal the reference's bit for bit.

:func:`cascade_autocorrelation` is the form a resident caller uses: all levels in one launch.  Input the device path
does not take (see :func:`_decline_reason`) runs the reference's function with a ``RuntimeWarning`` that says why; the
multivariate function is not offered.  This module does not import pysteps.
"""

import math
from fractions import Fraction

import numpy as np

from .. import _lib
from .._reference import decline, lookup
from ..device import DeviceArray

__all__ = ["temporal_autocorrelation", "cascade_autocorrelation"]

MAX_LAGS = 8  # csrc/autocorr.hip kAcMaxLags
MAX_RADIUS = 2048  # csrc/anvil.hip kAnvilMaxRadius
_RESOLVED = Fraction(1, 1 << 96)  # relative variance the double-double sums still tell from zero
_REAL = (np.dtype(np.float32), np.dtype(np.float64))


# ---- the host finish: exact rationals, one rounding --------------------------------------------------------------

def _exact(pair):
    """A double-double pair as the rational it stands for (None: not finite)."""
    hi, lo = float(pair[0]), float(pair[1])
    if not (math.isfinite(hi) and math.isfinite(lo)):
        return None
    return Fraction(hi) + Fraction(lo)


def _ratio_sqrt(num, den2):
    """``num / sqrt(den2)`` of two rationals (``den2 > 0``) as the nearest float64: the square root is taken to 128
    bits beyond the quotient's leading one before the one rounding."""
    if num == 0:
        return 0.0
    q = num * num / den2
    p_, q_ = q.numerator, q.denominator
    s = 128 + max(0, (q_.bit_length() - p_.bit_length()) // 2 + 1)
    root = Fraction(math.isqrt((p_ << (2 * s)) // q_), 1 << s)
    return float(-root if num < 0 else root)


def _corrcoef_from_sums(s_a, s_aa, s_b, s_bb, s_ab, count):
    """np.corrcoef(a, b)[0, 1] from the exact sums over ``count`` values; NaN as the reference gives it: fewer than
    two values, a constant plane."""
    if count < 2 or None in (s_a, s_aa, s_b, s_bb, s_ab):
        return float("nan")
    var_a = count * s_aa - s_a * s_a
    var_b = count * s_bb - s_b * s_b
    if var_a <= _RESOLVED * count * s_aa or var_b <= _RESOLVED * count * s_bb:
        return float("nan")
    return min(1.0, max(-1.0, _ratio_sqrt(count * s_ab - s_a * s_b, var_a * var_b)))


def _gamma_spatial(sums, count):
    """One level's coefficients from its sums (2 + 3 K, 2)."""
    K = (sums.shape[0] - 2) // 3
    s_a, s_aa = _exact(sums[0]), _exact(sums[1])
    return [_corrcoef_from_sums(s_a, s_aa, _exact(sums[2 + 3 * k]), _exact(sums[3 + 3 * k]), _exact(sums[4 + 3 * k]), count)
            for k in range(K)]


def _gamma_spectral(sums, corners):
    """One level's coefficients from its sums (1 + 2 K, 2) and the (differenced) series' DC coefficients, newest
    first (K + 1 complex): spectral.py:62-76 with the DC terms as the reference writes them, not clipped."""
    K = (sums.shape[0] - 1) // 2
    X0 = corners[0]
    s_d1 = _exact(sums[0])
    out = []
    for k in range(K):
        Y0 = corners[k + 1]
        s_n, s_d2 = _exact(sums[1 + 2 * k]), _exact(sums[2 + 2 * k])
        dc = (float(np.real(X0 * Y0)), float(np.real(X0) ** 2), float(np.real(Y0) ** 2))
        if None in (s_n, s_d1, s_d2) or not all(math.isfinite(v) for v in dc):
            out.append(float("nan"))
            continue
        n, d1, d2 = s_n - Fraction(dc[0]), s_d1 - Fraction(dc[1]), s_d2 - Fraction(dc[2])
        out.append(_ratio_sqrt(n, d1 * d2) if d1 * d2 > 0 else float("nan"))
    return out


# ---- the kernels -------------------------------------------------------------------------------------------------

def _download(dev, nsum_doubles, nwords):
    host = np.empty(nsum_doubles + nwords, dtype=np.float64)
    _lib.check(_lib.lib().psh_memcpy_d2h(host.ctypes.data, dev.ptr, host.nbytes), "psh_memcpy_d2h")
    return host[:nsum_doubles], host[nsum_doubles:].view(np.uint64)


def spatial_sums(stack, L, T, npix, mask, d):
    """``psh_autocorr_sums_dev`` on a float32 / float64 DeviceArray holding ``(L, T, npix)`` and a uint8 DeviceArray
    mask of ``npix`` bytes (or None): the sums ``(L, 2 + 3 K, 2)``, the masked pixel count and the non-finite counts
    ``(L,)`` on the host (waits)."""
    nsums = 2 + 3 * (T - d - 1)
    out = DeviceArray((L * nsums * 2 + 1 + L,), np.float64)
    _lib.check(_lib.lib().psh_autocorr_sums_dev(stack.ptr, int(stack.dtype == np.float64), L, T, npix,
                                                None if mask is None else mask.ptr, d, out.ptr,
                                                out.ptr + L * nsums * 16, out.ptr + L * nsums * 16 + 8), "psh_autocorr_sums_dev")
    sums, words = _download(out, L * nsums * 2, 1 + L)
    return sums.reshape(L, nsums, 2), int(words[0]), words[1:]


def spectral_sums(spectra, L, T, m, nc, n, use_full_fft, d):
    """``psh_autocorr_spectral_sums_dev`` on a complex128 DeviceArray holding ``(L, T, m, nc)``: the sums
    ``(L, 1 + 2 K, 2)`` and the non-finite counts ``(L,)`` on the host (waits)."""
    nsums = 1 + 2 * (T - d - 1)
    out = DeviceArray((L * nsums * 2 + L,), np.float64)
    _lib.check(_lib.lib().psh_autocorr_spectral_sums_dev(spectra.ptr, L, T, m, nc, n, int(bool(use_full_fft)), d, out.ptr,
                                                         out.ptr + L * nsums * 16), "psh_autocorr_spectral_sums_dev")
    sums, words = _download(out, L * nsums * 2, L)
    return sums.reshape(L, nsums, 2), words


def _corners(x, L, T, plane, d):
    """The DC coefficients ``x[l, t, 0, 0]`` as an (L, T' ) complex array, newest first, differenced like the series."""
    if isinstance(x, DeviceArray):
        c = np.empty((L, T), dtype=np.complex128)
        for i in range(L * T):
            _lib.check(_lib.lib().psh_memcpy_d2h(c.ctypes.data + 16 * i, x.ptr + 16 * plane * i, 16), "psh_memcpy_d2h")
    else:
        c = np.ascontiguousarray(x.reshape(L, T, plane)[:, :, 0])
    if d == 1:
        c = np.diff(c, axis=1)
    return c[:, ::-1]


def _window_planes(x, mask, d, window_radius):
    """The moving-window coefficients of a float64 DeviceArray ``(T, m, n)``: a list of ``(m, n)`` DeviceArrays."""
    from ..nowcasts.anvil import RECIPE_CORR, RECIPE_PLAIN, _plane, gaussian_filter_dev  # noqa: PLC0415

    lib = _lib.lib()
    T, m, n = x.shape
    npix = m * n
    prepared = DeviceArray((1 + T - d, m, n), np.float64)
    bad = DeviceArray((1,), np.uint64)
    _lib.check(lib.psh_autocorr_window_prepare_dev(x.ptr, T, npix, None if mask is None else mask.ptr, d, prepared.ptr, bad.ptr),
               "psh_autocorr_window_prepare_dev")
    if int(bad.to_host()[0]):
        raise ValueError("x contains non-finite values")
    factor = float(window_radius ** 2)
    newest = _plane(prepared, T - d)
    out = []
    for k in range(T - d - 1):
        older = _plane(prepared, T - d - 1 - k)
        plain = gaussian_filter_dev([_plane(prepared, 0), newest, older], window_radius, RECIPE_PLAIN)
        corr = gaussian_filter_dev([newest, older], window_radius, RECIPE_CORR)
        cc = DeviceArray((m, n), np.float64)
        f = [_plane(plain, j).ptr for j in range(3)] + [_plane(corr, j).ptr for j in range(3)]
        _lib.check(lib.psh_window_corrcoef_dev(f[0], f[1], f[2], f[3], f[4], f[5], factor, npix, cc.ptr), "psh_window_corrcoef_dev")
        out.append(cc)
    return out


# ---- the public functions ----------------------------------------------------------------------------------------

def _check_arguments(x, domain, mask):
    """correlation.py:94-105: the reference's checks and messages, in its order.  Needs no device."""
    if len(x.shape) < 2:
        raise ValueError("the dimension of x must be >= 2")
    if len(x.shape) != 3 and domain == "spectral":
        raise NotImplementedError(
            "len(x.shape[1:]) = %d, but with domain == 'spectral', this function has only been implemented for two-dimensional fields"
            % len(x.shape[1:])
        )
    if mask is not None and tuple(mask.shape) != tuple(x.shape[1:]):
        raise ValueError(
            "dimension mismatch between x and mask: x.shape[1:]=%s, mask.shape=%s"
            % (str(tuple(x.shape[1:])), str(tuple(mask.shape)))
        )


def _decline_reason(x, d, domain, mask, window_radius, lead=1):
    """Why the device path does not take this call (None: it does).  Needs no device.  ``lead``: the axes in front of
    the fields' own (1: a series, 2: a cascade)."""
    if not isinstance(x, (np.ndarray, DeviceArray)):
        return "x is neither a NumPy array nor a DeviceArray"
    if d not in (0, 1):
        return "d = %r" % (d,)
    lags = int(x.shape[lead - 1]) - d - 1
    if lags > MAX_LAGS:
        return "%d lags (more than %d)" % (lags, MAX_LAGS)
    if int(np.prod(x.shape[lead:], dtype=np.int64)) == 0:
        return "empty fields"
    dtype = np.dtype(x.dtype)
    if domain == "spectral":
        if dtype != np.complex128:
            return "dtype %s (the spectral path is complex128)" % dtype
    elif dtype not in _REAL:
        return "dtype %s (the device path is float32 / float64)" % dtype
    if mask is not None and domain != "spectral":
        if isinstance(mask, DeviceArray):
            if mask.dtype != np.uint8:
                return "a resident mask that is not uint8"
        elif not isinstance(mask, np.ndarray) or mask.dtype != np.bool_:
            return "a host mask that is not a boolean array"
    if domain != "spectral" and window_radius != np.inf:
        if len(x.shape) - lead != 2:
            return "moving-window input that is not two-dimensional"
        if dtype != np.float64:
            return "moving-window input of dtype %s (float64 is served)" % dtype
        if not (float(window_radius) > 0.0) or int(4.0 * float(window_radius) + 0.5) > MAX_RADIUS:
            return "window_radius=%s (Gaussian radius outside 0..%d)" % (window_radius, MAX_RADIUS)
    return None


def _resident(x, mask):
    return isinstance(x, DeviceArray) or isinstance(mask, DeviceArray)


def _upload(x):
    return x if isinstance(x, DeviceArray) else DeviceArray.from_host(np.ascontiguousarray(x), sync=False)


def _upload_mask(mask):
    if mask is None or isinstance(mask, DeviceArray):
        return mask
    return DeviceArray.from_host(np.ascontiguousarray(mask).view(np.uint8), sync=False)


def _no_lags(x):
    """A series too short for one lag: the reference's non-finite check, then nothing to correlate."""
    host = x.to_host() if isinstance(x, DeviceArray) else x
    if np.any(~np.isfinite(host)):
        raise ValueError("x contains non-finite values")


def _spectral_shape(x, x_shape, use_full_fft):
    m, nc = (int(s) for s in x.shape[-2:])
    n = nc if use_full_fft else int(x_shape[1])
    if not use_full_fft and nc != n // 2 + 1:
        raise ValueError("x_shape=%s does not belong to spectra of shape %s" % (str(tuple(x_shape)), str((m, nc))))
    return m, nc, n


def temporal_autocorrelation(x, d=0, domain="spatial", x_shape=None, mask=None, use_full_fft=False, window="gaussian",
                             window_radius=np.inf):
    """Lag-l temporal autocorrelation coefficients of a time series of fields (reference:
    pysteps/timeseries/correlation.py:21-130; parameters as documented there).  Returns a list of length
    ``x.shape[0] - d - 1``: Python floats, or with ``window_radius < inf`` arrays of ``x.shape[1:]``.

    ``x`` may be a float32 / float64 (spectral: complex128) :class:`~pysteps_amd.device.DeviceArray` and ``mask`` a
    uint8 one; they are read where they lie, and window planes then come back as ``DeviceArray`` s.  ``window`` is
    accepted and - like in the reference, which never passes it on (correlation.py:121) - ignored: the window is
    Gaussian."""
    _check_arguments(x, domain, mask)
    why = _decline_reason(x, d, domain, mask, window_radius)
    if why is not None:
        ref = decline("temporal_autocorrelation", why, lookup("timeseries.correlation", "temporal_autocorrelation",
                                                              temporal_autocorrelation), _resident(x, mask))
        return ref(x, d=d, domain=domain, x_shape=x_shape, mask=mask, use_full_fft=use_full_fft, window=window,
                   window_radius=window_radius)
    if int(x.shape[0]) - int(d) < 2:
        _no_lags(x)
        return []
    if domain == "spatial" and window_radius != np.inf:
        planes = _window_planes(_upload(x), _upload_mask(mask), int(d), window_radius)
        return planes if isinstance(x, DeviceArray) else [np.array(p.to_host()) for p in planes]
    return [float(v) for v in _cascade(x, 1, mask, int(d), domain, x_shape, use_full_fft)[0]]


def _cascade(x, lead, mask, d, domain, x_shape, use_full_fft):
    """(L, K) coefficients of ``x``: a series (``lead`` = 1, L = 1) or a cascade (``lead`` = 2)."""
    L = 1 if lead == 1 else int(x.shape[0])
    T = int(x.shape[lead - 1])
    if domain == "spatial":
        npix = int(np.prod(x.shape[lead:], dtype=np.int64))
        sums, count, bad = spatial_sums(_upload(x), L, T, npix, _upload_mask(mask), d)
        if bad.any():
            raise ValueError("x contains non-finite values")
        return np.array([_gamma_spatial(sums[l], count) for l in range(L)], dtype=np.float64)
    m, nc, n = _spectral_shape(x, x_shape, use_full_fft)
    sums, bad = spectral_sums(_upload(x), L, T, m, nc, n, use_full_fft, d)
    if bad.any():
        raise ValueError("x contains non-finite values")
    corners = _corners(x, L, T, m * nc, d)
    return np.array([_gamma_spectral(sums[l], corners[l]) for l in range(L)], dtype=np.float64)


def cascade_autocorrelation(cascades, mask=None, d=0, domain="spatial", x_shape=None, use_full_fft=False):
    """The autocorrelation coefficients of every level of a cascade ``(L, T, ...)`` - a NumPy array or a
    :class:`~pysteps_amd.device.DeviceArray` - from one launch: an ``(L, T - d - 1)`` float64 array whose rows are, bit
    for bit, what :func:`temporal_autocorrelation` gives level by level.  ``mask`` is shared by the levels."""
    if len(cascades.shape) < 3:
        raise ValueError("the dimension of cascades must be >= 3")
    if len(cascades.shape) != 4 and domain == "spectral":
        raise NotImplementedError(
            "len(cascades.shape[2:]) = %d, but with domain == 'spectral', this function has only been implemented for "
            "two-dimensional fields" % len(cascades.shape[2:])
        )
    if mask is not None and tuple(mask.shape) != tuple(cascades.shape[2:]):
        raise ValueError(
            "dimension mismatch between cascades and mask: cascades.shape[2:]=%s, mask.shape=%s"
            % (str(tuple(cascades.shape[2:])), str(tuple(mask.shape)))
        )
    why = _decline_reason(cascades, d, domain, mask, np.inf, lead=2)
    if why is not None:
        ref = decline("cascade_autocorrelation", why, lookup("timeseries.correlation", "temporal_autocorrelation",
                                                             temporal_autocorrelation), _resident(cascades, mask))
        return np.array([ref(cascades[l], d=d, domain=domain, x_shape=x_shape, mask=mask, use_full_fft=use_full_fft)
                         for l in range(cascades.shape[0])], dtype=np.float64)
    if int(cascades.shape[1]) - int(d) < 2:
        _no_lags(cascades)
        return np.empty((int(cascades.shape[0]), 0), dtype=np.float64)
    return _cascade(cascades, 2, mask, int(d), domain, x_shape, use_full_fft)
