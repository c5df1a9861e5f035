"""One step of the AR(p) model of a cascade level on the GPU (mirror of
pysteps/timeseries/autoregression.py:1020-1070, ``iterate_ar_model``).

The member loops call it once per member, cascade level and time step (pysteps/nowcasts/steps.py:1095,
1137, sprog.py:398, sseps.py:678,749, anvil.py:483).  ``psh_ar_iterate_dev`` evaluates the reference's
expression ``x_new = 0.0; x_new += phi[i] * x[-(i + 1)]; x_new += phi[-1] * eps`` with every product
rounded before it is added, so float64 results are bit-identical with NumPy's.

Device path: float64 series of at least two dimensions, scalar ``phi`` of order 1..8, ``eps`` of
``x.shape[1:]`` or None; ``DeviceArray`` in gives ``DeviceArray`` out (the form a resident member loop
uses).  Everything else - one-dimensional series, other dtypes, per-pixel ``phi``, small host arrays
(the transfer would cost more than NumPy's arithmetic) - runs the reference's function.

The estimate of the model is here too, so that a resident caller gets its AR parameters with no pysteps installed:
``adjust_lag2_corrcoef1`` / ``adjust_lag2_corrcoef2``, ``estimate_ar_params_yw`` and ``test_ar_stationarity`` are host
restatements of autoregression.py:31-78, 402-476 and 1138-1161 with the reference's NumPy calls in its order (a handful
of scalars per cascade level: the reference's bits and its error text), and :func:`cascade_ar_params` chains them
behind the device autocorrelation (:mod:`pysteps_amd.timeseries.correlation`) the way nowcasts/steps.py:834-866 does.
"""

import ctypes

import numpy as np

from .. import _lib
from .._reference import require
from ..device import DeviceArray

MAX_ORDER = 8
MIN_HOST_PLANE = 1 << 16  # host arrays below this many values per field stay with NumPy



def _stock():
    """The reference's function: its ImportError without pysteps, NotImplementedError if ours has taken its place."""
    return require("timeseries.autoregression", "iterate_ar_model", iterate_ar_model)


def _scalar_phi(phi):
    try:
        if not 2 <= len(phi) <= MAX_ORDER + 1:
            return None
        if any(np.ndim(v) != 0 for v in phi):
            return None
        return np.asarray(phi, dtype=np.float64)
    except TypeError:
        return None


def iterate_ar_model(x, phi, eps=None):
    """Apply an AR(p) model to a time series (parameters and return value as documented for the
    reference, autoregression.py:1021-1040)."""
    resident = isinstance(x, DeviceArray)
    coeffs = _scalar_phi(phi)
    eligible = (
        coeffs is not None and len(x.shape) >= 2 and x.dtype == np.float64
        and (eps is None or (isinstance(eps, (np.ndarray, DeviceArray)) and eps.dtype == np.float64))
    )
    if resident:
        if not eligible or (eps is not None and not isinstance(eps, DeviceArray)):
            raise NotImplementedError("device-resident series: float64, scalar phi of order 1..8, resident eps")
    elif not eligible or isinstance(eps, DeviceArray) or int(np.prod(x.shape[1:])) < MIN_HOST_PLANE:
        return _stock()(x, phi, eps=eps)
    if x.shape[0] < len(phi) - 1:  # autoregression.py:1041-1045
        raise ValueError(
            "dimension mismatch between x and phi: x.shape[0]=%d, len(phi)=%d" % (x.shape[0], len(phi))
        )
    if eps is not None and tuple(eps.shape) != tuple(x.shape[1:]):  # :1053-1057
        raise ValueError(
            "dimension mismatch between x and eps: x[1:].shape=%s, eps.shape=%s"
            % (str(tuple(x.shape[1:]) if resident else x[1:].shape), str(tuple(eps.shape)))
        )
    plane = int(np.prod(x.shape[1:]))
    if plane == 0:
        return _stock()(x, phi, eps=eps)
    d_x = x if resident else DeviceArray.from_host(x, np.float64, sync=False)
    d_eps = eps if resident or eps is None else DeviceArray.from_host(eps, np.float64, sync=False)
    out = DeviceArray(x.shape, np.float64)
    phi_c = (ctypes.c_double * coeffs.size)(*coeffs)
    _lib.check(
        _lib.lib().psh_ar_iterate_dev(d_x.ptr, int(x.shape[0]), plane, phi_c, coeffs.size - 1,
                                      None if d_eps is None else d_eps.ptr, out.ptr),
        "psh_ar_iterate_dev",
    )
    return out if resident else out.to_host()  # blocks are recycled in stream order: inputs may die now


# ---- the estimate of the model: host restatements (scalars per cascade level) ---------------------------------------

def adjust_lag2_corrcoef1(gamma_1, gamma_2):
    """The simple adjustment of the lag-2 coefficient that keeps the Yule-Walker AR(2) process stationary
    (autoregression.py:31-52)."""
    gamma_2 = np.maximum(gamma_2, 2 * gamma_1 * gamma_1 - 1 + 1e-10)
    return np.minimum(gamma_2, 1 - 1e-10)


def adjust_lag2_corrcoef2(gamma_1, gamma_2):
    """The more advanced adjustment of the lag-2 coefficient (autoregression.py:55-78)."""
    gamma_2 = np.maximum(gamma_2, 2 * gamma_1 * gamma_2 - 1)
    return np.maximum(gamma_2, (3 * gamma_1**2 - 2 + 2 * (1 - gamma_1**2) ** 1.5) / gamma_1**2)


def test_ar_stationarity(phi):
    """True if the roots of x^p - phi_1 x^(p-1) - ... lie inside the unit circle as the reference tests it
    (autoregression.py:1138-1161: the polynomial it hands to ``np.roots`` is ``[1, -phi_1, ..., -phi_(p-1)]``)."""
    moduli = np.array([np.abs(root) for root in np.roots([1.0 if i == 0 else -phi[i] for i in range(len(phi))])])
    return not np.any(moduli >= 1)


test_ar_stationarity.__test__ = False  # the reference's name; not a test


def _compute_differenced_model_params(phi, p, q, d):
    """The parameters of the integrated ARI(p, d) model from those of the differenced series, scalar case
    (autoregression.py:1199-1221 with q = 1; binom(1, 1) = 1)."""
    if q != 1 or d not in (0, 1):
        raise NotImplementedError("scalar AR models with d = 0 or 1")
    out = [0.0] * (p + d)
    for i in range(1, d + 1):
        out[i - 1] -= 1.0 * (-1) ** i
    for i in range(1, p + 1):
        out[i - 1] += phi[i - 1]
    for i in range(1, p + 1):
        for j in range(1, d + 1):
            out[i + j - 1] += phi[i - 1] * 1.0 * (-1) ** j
    return out


def estimate_ar_params_yw(gamma, d=0, check_stationarity=True):
    """The parameters phi_1 .. phi_p and the innovation term of an AR(p) model from the Yule-Walker equations
    (autoregression.py:402-476): an array of p + d + 1 values."""
    if d not in [0, 1]:
        raise ValueError("d = %d, but 0 or 1 required" % d)
    p = len(gamma)
    g = np.hstack([[1.0], gamma])
    G = np.array([np.roll(g[:-1], j) for j in range(p)])
    phi = np.linalg.solve(G, g[1:].flatten())
    if check_stationarity and not test_ar_stationarity(phi):
        raise RuntimeError("Error in estimate_ar_params_yw: nonstationary AR(p) process")
    c = 1.0
    for j in range(p):
        c -= gamma[j] * phi[j]
    phi_pert = 0.0 if c < 0 else np.sqrt(c)  # a negative radicand: no innovation term
    if d == 1:
        phi = _compute_differenced_model_params(phi, p, 1, 1)
    out = np.empty(len(phi) + 1)
    out[: len(phi)] = phi
    out[-1] = phi_pert
    return out


def cascade_ar_params(cascades, mask=None, ar_order=None, d=0, domain="spatial", x_shape=None, use_full_fft=False,
                      check_stationarity=True):
    """The chain of nowcasts/steps.py:834-866 for a cascade ``(L, T, ...)`` (NumPy or ``DeviceArray``): the
    autocorrelation coefficients of every level from one launch
    (:func:`pysteps_amd.timeseries.correlation.cascade_autocorrelation`), the lag-2 adjustment
    (:func:`adjust_lag2_corrcoef2`) when there are two lags, and Yule-Walker per level.  ``ar_order``: the lags to
    use (None: all ``T - d - 1``).  Returns ``(gamma, phi)``: ``(L, ar_order)`` and ``(L, ar_order + d + 1)``."""
    from .correlation import cascade_autocorrelation  # noqa: PLC0415

    gamma = cascade_autocorrelation(cascades, mask=mask, d=d, domain=domain, x_shape=x_shape, use_full_fft=use_full_fft)
    if ar_order is not None:
        if not 1 <= ar_order <= gamma.shape[1]:
            raise ValueError("ar_order = %d, but the cascade holds %d lags" % (ar_order, gamma.shape[1]))
        gamma = np.ascontiguousarray(gamma[:, :ar_order])
    if gamma.shape[1] == 2:
        for i in range(gamma.shape[0]):
            gamma[i, 1] = adjust_lag2_corrcoef2(gamma[i, 0], gamma[i, 1])
    phi = np.empty((gamma.shape[0], gamma.shape[1] + d + 1))
    for i in range(gamma.shape[0]):
        phi[i, :] = estimate_ar_params_yw(gamma[i, :], d=d, check_stationarity=check_stationarity)
    return gamma, phi
