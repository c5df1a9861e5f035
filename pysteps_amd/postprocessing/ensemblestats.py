"""Ensemble mean and exceedance probabilities on the device, mirror of ``pysteps.postprocessing.ensemblestats``
(reference: pysteps/postprocessing/ensemblestats.py ``mean`` :20-58, ``excprob`` :61-115).

``psh_ens_products_dev`` (csrc/ensstats.hip) reads a member stack ``(k, m, n)`` once and writes the mean plane and one
probability plane per threshold in the same pass, so the products come from the members where they lie:

* :func:`mean` and :func:`excprob` have the reference's signatures, checks, exception texts, shapes and dtypes.  A
  NumPy stack is uploaded and a NumPy result returned; a :class:`~pysteps_amd.device.DeviceArray` gives a
  ``DeviceArray`` and no host transfer.  float32 and float64 stacks run on the device; other dtypes go to the
  reference with a warning if pysteps is importable, else raise.
* :func:`products` is the fused form: ``(mean, probs)`` of one pass (16 thresholds per pass).
* :class:`EnsembleProducts` accumulates both per lead time and serves as the ``callback`` of a nowcast; with
  ``pysteps_amd.nowcasts.utils.nowcast_main_loop`` it receives the advected members as a ``DeviceArray``
  (``accepts_device``), so with ``return_output=False`` no member crosses the bus.

The arithmetic is the reference's, operation by operation: NumPy reduces a C-contiguous ``(k, m, n)`` stack along
axis 0 in member order, in the stack's own type; a thread of the kernel owns a pixel for all members and adds in that
order.  The results are bit-identical with the reference's (tests/test_ensstats_gpu.py).  A threshold is compared as
NumPy compares it: a Python number meets a float32 stack as float32, a ``numpy.float64`` scalar as float64 (NumPy's
promotion rules, asked through ``numpy.result_type``).

``banddepth`` has no device version on purpose: the reference breaks ties with unseeded ``np.random.random`` (:163-164),
and precipitation ensembles are mostly ties (dry pixels), so its result is not a function of its input and nothing
could hold a device version to it.
"""

import ctypes
import warnings

import numpy as np

from .. import _lib
from .._reference import decline, lookup
from ..device import DeviceArray, _compared_as, _dtype_of

__all__ = ["mean", "excprob", "products", "EnsembleProducts"]

MAX_THRESHOLDS = 16  # csrc/ensstats.hip kEnsMaxThr: thresholds per pass over the members
_NATIVE = (np.dtype(np.float32), np.dtype(np.float64))


def _stock(name):
    """The reference's ``mean`` / ``excprob``, or None when pysteps is not importable."""
    return lookup("postprocessing.ensemblestats", name, globals()[name])


def _stack(X, k, plane_shape):
    """(device stack, k, plane shape) of a DeviceArray or a host array, uploaded as it is."""
    if isinstance(X, DeviceArray):
        return X
    return DeviceArray.from_host(np.ascontiguousarray(np.asarray(X)).reshape((k,) + tuple(plane_shape)), sync=False)


def _run(dev, k, plane_shape, thresholds, prob_ignore_nan, want_mean, mean_ignore_nan, mean_thr, widen):
    """One pass per 16 thresholds over the device stack ``dev`` of ``k`` planes.  ``thresholds`` / ``mean_thr`` are the
    float64 numbers of :func:`_compared_as`.  Returns (mean DeviceArray or None, probs DeviceArray (T, ...) or None)."""
    npix = int(np.prod(plane_shape, dtype=np.int64))
    if dev.dtype not in _NATIVE:
        raise NotImplementedError("ensemble products on the device: float32 or float64 members, not %s" % dev.dtype)
    f64 = dev.dtype == np.float64
    lib = _lib.lib()
    mean_out = None
    if want_mean:
        mean_out = DeviceArray(plane_shape, np.float64 if (f64 or widen) else np.float32)
    T = len(thresholds)
    probs = DeviceArray((T,) + tuple(plane_shape), np.float64) if T else None
    thr = np.ascontiguousarray(thresholds, dtype=np.float64)
    first = True
    for t0 in range(0, max(T, 1), MAX_THRESHOLDS):
        n = min(MAX_THRESHOLDS, T - t0)
        mean_ptr = mean_out.ptr if (first and mean_out is not None) else None
        if n <= 0 and mean_ptr is None:
            break
        _lib.check(
            lib.psh_ens_products_dev(dev.ptr, int(f64), int(k), npix, thr[t0:].ctypes.data_as(ctypes.c_void_p) if n > 0 else None,
                                     max(n, 0), int(bool(prob_ignore_nan)), int(bool(mean_ignore_nan)),
                                     int(mean_thr is not None), float(mean_thr) if mean_thr is not None else 0.0,
                                     int(bool(widen)), mean_ptr, probs.ptr + t0 * npix * 8 if n > 0 else None),
            "psh_ens_products_dev",
        )
        first = False
    for out in (mean_out, probs):
        if out is not None:
            out._keep = (dev, dev._keep)  # the stack (and a host buffer still being uploaded) outlives the queued pass
    return mean_out, probs


def _check_mean(X):
    shape = tuple(X.shape) if isinstance(X, DeviceArray) else np.asanyarray(X).shape
    ndim = len(shape)
    if ndim > 3 or ndim <= 1:
        raise Exception("Number of dimensions of X should be 2 or 3." + "It was: {}".format(ndim))
    return ((1,) + shape) if ndim == 2 else shape


def _check_excprob(X):
    shape = tuple(X.shape) if isinstance(X, DeviceArray) else np.asanyarray(X).shape
    if len(shape) < 3:
        raise Exception(f"Number of dimensions of X should be 3 or more. It was: {len(shape)}")
    return shape


def _threshold_list(X_thr):
    if np.isscalar(X_thr):
        return [X_thr], True
    return list(X_thr), False


def mean(X, ignore_nan=False, X_thr=None):
    """Ensemble mean of ``X`` ``(k, m, n)`` (or one field ``(m, n)``) -> ``(m, n)``, in the stack's dtype; parameters as
    documented in the reference (ensemblestats.py:20-39).  ``ignore_nan`` ignores NaN, ``X_thr`` also values below it."""
    shape = _check_mean(X)
    dtype = _dtype_of(X)
    resident = isinstance(X, DeviceArray)
    if dtype not in _NATIVE:
        return decline("ensemblestats.mean", "dtype %s" % dtype, _stock("mean"), resident, UserWarning)(
            X, ignore_nan=ignore_nan, X_thr=X_thr)
    thr = None if X_thr is None else _compared_as(X_thr, dtype)
    out, _ = _run(_stack(X, shape[0], shape[1:]), shape[0], shape[1:], [], False, True, ignore_nan, thr, False)
    return out if resident else out.to_host()


def excprob(X, X_thr, ignore_nan=False):
    """Exceedance probabilities of ``X`` ``(k, m, n, ...)`` for the threshold(s) ``X_thr`` -> float64
    ``(len(X_thr), m, n, ...)``, without the first axis for a scalar threshold (ensemblestats.py:61-115)."""
    shape = _check_excprob(X)
    dtype = _dtype_of(X)
    resident = isinstance(X, DeviceArray)
    if dtype not in _NATIVE:
        return decline("ensemblestats.excprob", "dtype %s" % dtype, _stock("excprob"), resident, UserWarning)(
            X, X_thr, ignore_nan=ignore_nan)
    thresholds, scalar = _threshold_list(X_thr)
    if not thresholds:
        return np.stack([])  # the reference's own ValueError for an empty list
    thr = [_compared_as(x, dtype) for x in thresholds]
    _, probs = _run(_stack(X, shape[0], shape[1:]), shape[0], shape[1:], thr, ignore_nan, False, False, None, False)
    if scalar:
        probs = probs.view(0)
    return probs if resident else probs.to_host()


def products(X, thresholds, *, mean=True, ignore_nan=False, mean_ignore_nan=False, mean_thr=None):
    """``(mean(X, mean_ignore_nan, mean_thr), excprob(X, thresholds, ignore_nan))`` from ONE pass over the members
    (one pass per 16 thresholds).  ``mean=False`` gives ``(None, probs)``; NumPy in, NumPy out; ``DeviceArray`` in,
    ``DeviceArray`` out."""
    return _products(X, thresholds, mean, ignore_nan, mean_ignore_nan, mean_thr, False)


def _products(X, thresholds, mean, ignore_nan, mean_ignore_nan, mean_thr, _widen):
    """:func:`products`; ``_widen``: float32 members are summed and compared as their float64 values."""
    shape = _check_excprob(X)
    want_mean = bool(mean)
    if want_mean and len(shape) != 3:
        _check_mean(X)
    dtype = _dtype_of(X)
    if dtype not in _NATIVE:
        ref_mean, ref_excprob = _stock("mean"), _stock("excprob")
        if ref_mean is None or ref_excprob is None or isinstance(X, DeviceArray):
            raise NotImplementedError("pysteps_amd ensemblestats.products: dtype %s is not implemented on the device" % dtype)
        warnings.warn("pysteps_amd ensemblestats.products: dtype %s - running the reference's functions" % dtype, stacklevel=3)
        return (ref_mean(X, mean_ignore_nan, mean_thr) if want_mean else None), ref_excprob(X, thresholds, ignore_nan)
    resident = isinstance(X, DeviceArray)
    thr_list, scalar = _threshold_list(thresholds)
    if not thr_list and not want_mean:
        raise ValueError("products: no threshold and no mean requested")
    as_dtype = np.dtype(np.float64) if _widen else dtype
    thr = [_compared_as(x, as_dtype) for x in thr_list]
    mthr = None if mean_thr is None else _compared_as(mean_thr, as_dtype)
    m_out, probs = _run(_stack(X, shape[0], shape[1:]), shape[0], shape[1:], thr, ignore_nan, want_mean, mean_ignore_nan,
                        mthr, _widen)
    if probs is not None and scalar:
        probs = probs.view(0)
    if resident:
        return m_out, probs
    return (None if m_out is None else m_out.to_host()), (None if probs is None else probs.to_host())


class EnsembleProducts:
    """Streaming accumulator of the ensemble products, usable as the ``callback`` of a nowcast::

        prod = EnsembleProducts([0.1, 1.0, 5.0])
        nowcasts.get_method("steps")(..., callback=prod, return_output=False)
        prod.mean       # (n_leadtimes, m, n)
        prod.excprob    # (n_leadtimes, T, m, n)

    Every call with the advected members of one lead time - a ``DeviceArray`` ``(k, m, n)`` or a host ``ndarray`` -
    appends one mean plane and one ``(T, m, n)`` probability block (options as :func:`products`).  float32 members are
    accumulated as float64: the block a nowcast returns is the float32 members widened, which is exact, so the products
    are bit-identical with the reference's ``mean`` / ``excprob`` of that block, and the mean is always float64.  The
    member stack is only read during the call (the advector may reuse it afterwards).

    ``keep="host"`` queues one copy per product into pinned memory (``psh_memcpy_d2h_async``) and waits for all of
    them when a result is first read; ``keep="device"`` keeps ``DeviceArray`` planes and returns stacked ``DeviceArray``s.
    """

    accepts_device = True

    def __init__(self, thresholds, *, mean=True, ignore_nan=False, mean_ignore_nan=False, mean_thr=None, keep="host"):
        if keep not in ("host", "device"):
            raise ValueError("keep must be 'host' or 'device', not %r" % (keep,))
        self.thresholds = [thresholds] if np.isscalar(thresholds) else list(thresholds)
        if not self.thresholds and not mean:
            raise ValueError("EnsembleProducts: no threshold and no mean requested")
        self._opts = dict(mean=bool(mean), ignore_nan=ignore_nan, mean_ignore_nan=mean_ignore_nan, mean_thr=mean_thr)
        self.keep = keep
        self._means, self._probs = [], []
        self._pending = False
        self.n_leadtimes = 0
        self.received = []  # type of the members of every call: DeviceArray or ndarray

    def __call__(self, members):
        resident = isinstance(members, DeviceArray)
        self.received.append(DeviceArray if resident else np.ndarray)
        if not resident:
            members = np.asarray(members)
        if len(members.shape) != 3:
            raise ValueError("EnsembleProducts: members of shape (k, m, n) expected, got %s" % (tuple(members.shape),))
        dev = members if resident else DeviceArray.from_host(np.ascontiguousarray(members), sync=False)
        o = self._opts
        m_out, probs = _products(dev, self.thresholds, o["mean"], o["ignore_nan"], o["mean_ignore_nan"], o["mean_thr"],
                                 dev.dtype == np.float32)
        if self.keep == "host":
            m_out, probs = self._queue_copy(m_out), self._queue_copy(probs)
        if m_out is not None:
            self._means.append(m_out)
        if probs is not None:
            self._probs.append(probs)
        self.n_leadtimes += 1

    def _queue_copy(self, dev):
        if dev is None:
            return None
        from .. import _pinned  # noqa: PLC0415

        host = _pinned.empty(dev.shape, dev.dtype)
        _lib.check(_lib.lib().psh_memcpy_d2h_async(host.ctypes.data, dev.ptr, dev.nbytes), "psh_memcpy_d2h_async")
        self._pending = True
        return host  # `dev` goes back to the stream-ordered block cache behind the queued copy

    def _stacked(self, planes):
        if not planes:
            return None
        if self.keep == "host":
            if self._pending:
                _lib.check(_lib.lib().psh_sync(), "psh_sync")
                self._pending = False
            return np.stack(planes)
        out = DeviceArray((len(planes),) + planes[0].shape, planes[0].dtype)
        for i, p in enumerate(planes):
            _lib.check(_lib.lib().psh_memcpy_d2d(out.ptr + i * p.nbytes, p.ptr, p.nbytes), "psh_memcpy_d2d")
        return out

    @property
    def mean(self):
        """``(n_leadtimes, m, n)`` float64, or None without ``mean``."""
        return self._stacked(self._means)

    @property
    def excprob(self):
        """``(n_leadtimes, T, m, n)`` float64, or None without thresholds."""
        return self._stacked(self._probs)
