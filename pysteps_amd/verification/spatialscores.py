"""The fractions skill score on the device, mirror of ``pysteps.verification.spatialscores`` ``fss``, ``fss_init``,
``fss_accum``, ``fss_merge`` and ``fss_compute`` (reference: pysteps/verification/spatialscores.py:516-677).

The reference thresholds both fields (finite and ``>= thr``), averages the 0/1 maps with
``scipy.ndimage.uniform_filter(size=scale, mode="constant")`` and adds ``sum(S_f**2)``, ``sum(S_f * S_o)`` and
``sum(S_o**2)`` to the FSS object.  ``S = c / scale**2`` with ``c`` the number of ones in the window, so the three sums
are integers over ``scale**4``; ``psh_fss_sums_dev`` (csrc/fss.hip) counts those integers - exact, the same in every
run - and this module divides once, in exact Python integers with one correctly rounded division.  The float filter of
the reference is then the side that carries the rounding error (tests/test_fss_cpu.py measures it).

* :func:`fss`, :func:`fss_init`, :func:`fss_accum`, :func:`fss_merge`, :func:`fss_compute`: the reference's signatures,
  shape check, messages and dict keys; objects of either implementation merge and compute interchangeably.  NumPy
  fields are uploaded, :class:`~pysteps_amd.device.DeviceArray` fields are used where they lie.
* :func:`fss_table`: the batched call the kernel is built for - a stack of forecasts, several thresholds and several
  scales at once.
* :class:`FssAccumulator`: a nowcast ``callback`` that scores the members of every lead time where they lie.

A threshold is compared as NumPy compares it: a Python number meets a float32 field as float32, a ``numpy.float64``
scalar as float64 (``device.py::_compared_as``).  What the device path does not take (another
dtype, a scale that is not an integer or exceeds 255, a side above 65535 pixels, a threshold so large that
``thr - 1 == thr``) goes to the reference with a warning when pysteps is importable and raises ``NotImplementedError``
otherwise.
"""

import ctypes
import warnings

import numpy as np

from .. import _lib
from .._reference import decline, lookup
from ..device import DeviceArray, _compared_as, _dtype_of, _upload

__all__ = ["fss", "fss_init", "fss_accum", "fss_merge", "fss_compute", "fss_table", "FssAccumulator", "MAX_SCALE", "MAX_SIDE"]

MAX_SCALE = 255  # csrc/fss.hip kFssMaxScale
MAX_SIDE = 65535  # csrc/fss.hip kFssMaxDim
_NATIVE = (np.dtype(np.float32), np.dtype(np.float64))
_SHAPE_MESSAGE = "X_f and X_o must be two-dimensional arrays having the same shape"


def _window(scale):
    """The integer window size the reference filters with: 1 (no filter) for ``scale <= 1``."""
    return int(scale) if scale > 1 else 1


def _unsupported(dtypes, shape, thrs, scales):
    for dtype in dtypes:
        if dtype not in _NATIVE:
            return "dtype %s" % dtype
    if max(shape[-2:]) > MAX_SIDE:
        return "a %d x %d field (at most %d pixels each way)" % (shape[-2], shape[-1], MAX_SIDE)
    for s in scales:
        try:
            ok = not s > 1 or (float(s) == int(s) and int(s) <= MAX_SCALE)
        except (TypeError, ValueError, OverflowError):
            ok = False
        if not ok:
            return "scale %r (an integer up to %d)" % (s, MAX_SCALE)
    for thr in thrs:
        for dtype in dtypes:
            try:
                # the reference marks non-finite pixels with thr - 1: they count as "below" only while that is below thr
                with np.errstate(all="ignore"):
                    below = np.asarray(thr - 1).astype(dtype)
                    separated = not bool(below >= thr)
            except Exception:
                separated = False
            if not separated:
                return "threshold %r (not above threshold - 1 as %s)" % (thr, dtype)
    return None


def _sums(dev_f, dev_o, K, m, n, shared, thr_f, thr_o, scales):
    """The integer sums ``(K, nthr, nsc, 3)`` uint64 of device fields; thresholds are the float64 numbers to compare
    with, scales the reference's (``<= 1``: no window)."""
    tf = np.ascontiguousarray(thr_f, dtype=np.float64)
    to = np.ascontiguousarray(thr_o, dtype=np.float64)
    sc = np.ascontiguousarray([float(s) for s in scales], dtype=np.float64)
    out = DeviceArray((K, tf.size, sc.size, 3), np.uint64)
    _lib.check(
        _lib.lib().psh_fss_sums_dev(dev_f.ptr, int(dev_f.dtype == np.float64), dev_o.ptr, int(dev_o.dtype == np.float64),
                                    int(bool(shared)), int(K), int(m), int(n), tf.ctypes.data_as(ctypes.c_void_p),
                                    to.ctypes.data_as(ctypes.c_void_p), int(tf.size), sc.ctypes.data_as(ctypes.c_void_p),
                                    int(sc.size), out.ptr),
        "psh_fss_sums_dev",
    )
    return np.array(out.to_host())  # the copy waits for the kernels: the fields may go after it


def _as_sum(count, window):
    """``count / window**4``: exact integers, one correctly rounded division (what the reference's sum approximates)."""
    return np.float64(int(count) / window**4)


def fss(X_f, X_o, thr, scale):
    """Compute the fractions skill score (FSS) for a deterministic forecast field ``X_f`` (m, n) and the corresponding
    observation field ``X_o`` (m, n), for the intensity threshold ``thr`` and the spatial scale ``scale`` in pixels
    (reference: spatialscores.py:516-546).  Returns the score, a float between 0 and 1 (NaN with a RuntimeWarning when
    neither field reaches the threshold anywhere)."""
    obj = fss_init(thr, scale)
    fss_accum(obj, X_f, X_o)
    return fss_compute(obj)


def fss_init(thr, scale):
    """Initialize a fractions skill score (FSS) verification object: the reference's dict (spatialscores.py:549-569)."""
    return dict(thr=thr, scale=scale, sum_fct_sq=0.0, sum_fct_obs=0.0, sum_obs_sq=0.0)


def fss_accum(fss, X_f, X_o):
    """Accumulate the forecast-observation pair ``X_f``, ``X_o`` (both (m, n), NumPy or DeviceArray) to the FSS object
    ``fss`` made by :func:`fss_init` (or by the reference's)."""
    if len(X_f.shape) != 2 or len(X_o.shape) != 2 or tuple(X_f.shape) != tuple(X_o.shape):
        raise ValueError(_SHAPE_MESSAGE)
    thr, scale = fss["thr"], fss["scale"]
    dt_f, dt_o = _dtype_of(X_f), _dtype_of(X_o)
    why = _unsupported((dt_f, dt_o), tuple(X_f.shape), [thr], [scale])
    if why is not None:
        resident = isinstance(X_f, DeviceArray) or isinstance(X_o, DeviceArray)
        return decline("fss_accum", why, lookup("verification.spatialscores", "fss_accum", fss_accum), resident,
                       UserWarning)(fss, X_f, X_o)
    m, n = X_f.shape
    counts = _sums(_upload(X_f), _upload(X_o), 1, m, n, True, [_compared_as(thr, dt_f)], [_compared_as(thr, dt_o)],
                   [scale])[0, 0, 0]
    w = _window(scale)
    fss["sum_obs_sq"] += _as_sum(counts[2], w)
    fss["sum_fct_obs"] += _as_sum(counts[1], w)
    fss["sum_fct_sq"] += _as_sum(counts[0], w)


def fss_merge(fss_1, fss_2):
    """Merge two FSS objects (spatialscores.py:613-654); returns the merged object."""
    if fss_1["thr"] != fss_2["thr"]:
        raise ValueError("cannot merge: the thresholds are not same %s!=%s" % (fss_1["thr"], fss_2["thr"]))
    if fss_1["scale"] != fss_2["scale"]:
        raise ValueError("cannot merge: the scales are not same %s!=%s" % (fss_1["scale"], fss_2["scale"]))
    fss = fss_1.copy()
    fss["sum_obs_sq"] += fss_2["sum_obs_sq"]
    fss["sum_fct_obs"] += fss_2["sum_fct_obs"]
    fss["sum_fct_sq"] += fss_2["sum_fct_sq"]
    return fss


def fss_compute(fss):
    """Compute the FSS of an FSS object (spatialscores.py:657-677)."""
    numer = fss["sum_fct_sq"] - 2.0 * fss["sum_fct_obs"] + fss["sum_obs_sq"]
    denom = fss["sum_fct_sq"] + fss["sum_obs_sq"]
    return 1.0 - numer / denom


def _table_sums(X_f, X_o, thrs, scales, widen):
    """uint64 ``(K, nthr, nsc, 3)`` of a stack ``(K, m, n)`` (or one field) against a plane or a matching stack;
    ``widen``: float32 forecasts are compared as their float64 values."""
    shape_f, shape_o = tuple(X_f.shape), tuple(X_o.shape)
    if len(shape_f) == 2:
        shape_f = (1,) + shape_f
    if len(shape_f) != 3 or shape_o not in (shape_f, shape_f[1:]):
        raise ValueError("X_f must have shape (m, n) or (K, m, n) and X_o shape (m, n) or that of X_f")
    K, m, n = shape_f
    shared = len(shape_o) == 2 or K == 1
    dt_f, dt_o = _dtype_of(X_f), _dtype_of(X_o)
    why = _unsupported((dt_f, dt_o), shape_f, thrs, scales)
    if why is not None:
        raise NotImplementedError("pysteps_amd fss_table: %s is not implemented on the device" % why)
    as_f = np.dtype(np.float64) if widen else dt_f
    return _sums(_upload(X_f), _upload(X_o), K, m, n, shared, [_compared_as(t, as_f) for t in thrs],
                 [_compared_as(t, dt_o) for t in thrs], scales)


def _scores(counts, scales):
    """FSS ``(..., nsc)`` of integer sums ``(..., nsc, 3)``, through the same float64 sums as :func:`fss`."""
    sums = np.empty(counts.shape, dtype=np.float64)
    for j, s in enumerate(scales):
        w = _window(s)
        flat = counts[..., j, :].reshape(-1)
        sums[..., j, :] = np.array([_as_sum(c, w) for c in flat.tolist()], dtype=np.float64).reshape(counts[..., j, :].shape)
    return fss_compute(dict(sum_fct_sq=sums[..., 0], sum_fct_obs=sums[..., 1], sum_obs_sq=sums[..., 2]))


def fss_table(X_f, X_o, thrs, scales, return_sums=False):
    """The FSS of every forecast of ``X_f`` - ``(K, m, n)``, or one field ``(m, n)`` - against ``X_o`` - one observation
    ``(m, n)`` shared by all of them, or a stack like ``X_f`` - for every threshold of ``thrs`` and every scale of
    ``scales``, in one call: float64 ``(K, nthr, nsc)``, or ``(nthr, nsc)`` for a single field, each entry equal to
    ``fss(X_f[k], X_o, thr, scale)``.  ``return_sums=True`` returns ``(scores, counts)``, ``counts`` the exact integers
    ``(..., 3)`` uint64: ``sum(c_f**2)``, ``sum(c_f * c_o)`` and ``sum(c_o**2)`` of the window counts (the reference's
    sums are these over ``scale**4``).  NumPy or DeviceArray fields, float32 or float64."""
    thrs = [thrs] if np.isscalar(thrs) else list(thrs)
    scales = [scales] if np.isscalar(scales) else list(scales)
    if not thrs or not scales:
        raise ValueError("fss_table: no threshold or no scale given")
    counts = _table_sums(X_f, X_o, thrs, scales, False)
    if len(X_f.shape) == 2:
        counts = counts[0]
    scores = _scores(counts, scales)
    return (scores, counts) if return_sums else scores


class FssAccumulator:
    """Streaming FSS of a nowcast against the observations of its lead times, usable as the ``callback`` of a nowcast::

        acc = FssAccumulator(observations, [0.1, 1.0, 5.0], [1, 4, 16, 64])
        nowcasts.get_method("steps")(..., callback=acc, return_output=False)
        acc.fss            # (n_leadtimes, nthr, nsc)
        acc.objects[t][i][j]  # the FSS object of lead time t, threshold i, scale j

    ``observations`` is ``(n_leadtimes, m, n)``, NumPy or DeviceArray, and is kept on the device.  Call ``t`` receives
    the members of lead time ``t`` - a ``DeviceArray`` ``(k, m, n)`` from the resident nowcast loop, a host ``ndarray``
    from any other - and scores every member against ``observations[t]``; the sums of the members are pooled into one
    FSS object per lead time, threshold and scale, in member order, exactly as a loop of :func:`fss_accum` over the
    members does.  float32 device members are compared as their float64 values: the block a nowcast returns is the
    float32 members widened, so the objects equal those of :func:`fss_accum` over that block.
    ``per_member=True`` also keeps every member's own score (``member_fss``)."""

    accepts_device = True

    def __init__(self, observations, thrs, scales, per_member=False):
        self.thrs = [thrs] if np.isscalar(thrs) else list(thrs)
        self.scales = [scales] if np.isscalar(scales) else list(scales)
        if not self.thrs or not self.scales:
            raise ValueError("FssAccumulator: no threshold or no scale given")
        if len(observations.shape) != 3:
            raise ValueError("FssAccumulator: observations of shape (n_leadtimes, m, n) expected, got %s"
                             % (tuple(observations.shape),))
        self._obs = observations if isinstance(observations, DeviceArray) else DeviceArray.from_host(np.asarray(observations))
        self.per_member = bool(per_member)
        self.objects = []
        self._member_fss = []
        self.n_leadtimes = 0
        self.received = []  # type of the members of every call: DeviceArray or ndarray

    def __call__(self, members):
        resident = isinstance(members, DeviceArray)
        self.received.append(DeviceArray if resident else np.ndarray)
        if not resident:
            members = np.asarray(members)
        if len(members.shape) != 3 or tuple(members.shape[1:]) != self._obs.shape[1:]:
            raise ValueError("FssAccumulator: members of shape (k, %d, %d) expected, got %s"
                             % (self._obs.shape[1:] + (tuple(members.shape),)))
        if self.n_leadtimes >= self._obs.shape[0]:
            raise ValueError("FssAccumulator: called for more lead times than the %d observations" % self._obs.shape[0])
        counts = _table_sums(members, self._obs.view(self.n_leadtimes), self.thrs, self.scales, resident)
        objects = [[fss_init(thr, scale) for scale in self.scales] for thr in self.thrs]
        for k in range(counts.shape[0]):
            for i in range(len(self.thrs)):
                for j, scale in enumerate(self.scales):
                    w, obj, c = _window(scale), objects[i][j], counts[k, i, j]
                    obj["sum_obs_sq"] += _as_sum(c[2], w)
                    obj["sum_fct_obs"] += _as_sum(c[1], w)
                    obj["sum_fct_sq"] += _as_sum(c[0], w)
        self.objects.append(objects)
        if self.per_member:
            with np.errstate(invalid="ignore"), warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                self._member_fss.append(_scores(counts, self.scales))
        self.n_leadtimes += 1

    @property
    def fss(self):
        """float64 ``(n_leadtimes, nthr, nsc)``: the pooled score of every lead time (NaN where nothing reached the
        threshold)."""
        out = np.empty((self.n_leadtimes, len(self.thrs), len(self.scales)), dtype=np.float64)
        with np.errstate(invalid="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            for t, objects in enumerate(self.objects):
                for i, row in enumerate(objects):
                    for j, obj in enumerate(row):
                        out[t, i, j] = fss_compute(obj)
        return out

    @property
    def member_fss(self):
        """float64 ``(n_leadtimes, k, nthr, nsc)`` with ``per_member=True``, else None."""
        return np.stack(self._member_fss) if self._member_fss else None
