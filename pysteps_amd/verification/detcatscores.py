"""Deterministic categorical scores on the device, mirror of ``pysteps.verification.detcatscores`` ``det_cat_fct``,
``det_cat_fct_init``, ``det_cat_fct_accum``, ``det_cat_fct_merge`` and ``det_cat_fct_compute`` (reference:
pysteps/verification/detcatscores.py).

The reference evaluates ``pred > thr`` and ``obs > thr`` with NaN comparing false - a NaN pixel is "no event" on its
side, it is not left out - and adds the numbers of hits, misses, false alarms and correct negatives to the contingency
table object.  ``psh_detcat_counts_dev`` (csrc/detscores.hip) counts them for a stack of forecasts and several
thresholds in one read: exact integers, the same in every run.  ``_merge`` and ``_compute`` are host arithmetic on a
handful of numbers, restated operation by operation, so a table holds the reference's bits.

* :func:`det_cat_fct`, :func:`det_cat_fct_init`, :func:`det_cat_fct_accum`, :func:`det_cat_fct_merge`,
  :func:`det_cat_fct_compute`: the reference's signatures, checks, messages, dict keys and dtypes; objects of either
  implementation accumulate, merge and compute interchangeably.  Like the reference's, ``det_cat_fct_merge`` copies the
  dict of its first argument, not its arrays: the count arrays of ``contab_1`` receive the sums.
* :func:`det_cat_table`: a stack of forecasts against one observation or a stack, several thresholds, one call.

Served on the device: ``axis=None`` (all elements) and, for ``(K, m, n)`` fields, the two trailing axes (``axis=(1, 2)``
or ``(2, 1)``), float32 or float64 on either side.  A threshold meets each field as NumPy compares it
(``device.py::_compared_as``).  Any other axis - the negative ones too, which in the reference
mean "no integration" - and any other dtype goes to the reference's function with a ``RuntimeWarning`` when pysteps is
importable and the fields are NumPy arrays, and raises ``NotImplementedError`` otherwise.
"""

import collections.abc
import ctypes

import numpy as np

from .. import _lib
from .._reference import decline, lookup
from ..device import DeviceArray, _compared_as, _dtype_of, _upload

__all__ = ["det_cat_fct", "det_cat_fct_init", "det_cat_fct_accum", "det_cat_fct_merge", "det_cat_fct_compute", "det_cat_table"]

_NATIVE = (np.dtype(np.float32), np.dtype(np.float64))
_COUNT_KEYS = ("hits", "misses", "false_alarms", "correct_negatives")  # the order of the kernel's four counts
def _as_iterable_axis(x):
    if x is None or (isinstance(x, collections.abc.Iterable) and not isinstance(x, int)):
        return x
    return (x,)


def _as_iterable_scores(x):
    if isinstance(x, collections.abc.Iterable) and not isinstance(x, str):
        return x
    return (x,)


def _check_fields(pred, obs, axis):
    """The reference's two checks, with its messages; returns the axes the scores are integrated over."""
    shape_p, shape_o = tuple(pred.shape), tuple(obs.shape)
    axis = tuple(range(len(shape_p))) if axis is None else axis
    if shape_p != shape_o:
        raise ValueError("the shape of pred does not match the shape of obs %s!=%s" % (shape_p, shape_o))
    if len(shape_p) <= np.max(axis):
        raise ValueError("axis %d is out of bounds for array of dimension %d" % (np.max(axis), len(shape_p)))
    return axis


def _layout(shape, axis, dtypes):
    """``(K, npix, shape of the object's arrays)`` of fields of ``shape`` integrated over ``axis`` on the device, or the
    reason why the device path declines."""
    for dtype in dtypes:
        if dtype not in _NATIVE:
            return None, "dtype %s" % dtype
    npix = int(np.prod(shape, dtype=np.int64))
    if npix < 1:
        return None, "an empty field"
    try:
        axes = sorted(int(a) for a in axis)
    except (TypeError, ValueError):
        return None, "axis %r" % (axis,)
    # the shape of the object's arrays as the reference forms it (NumPy integers: its messages print them)
    nshape = tuple(np.array(shape)[np.array([dim not in axes for dim in range(len(shape))], dtype=bool)])
    if axes == list(range(len(shape))):
        return (1, npix, nshape), None
    if len(shape) == 3 and axes == [1, 2]:
        return (shape[0], shape[1] * shape[2], nshape), None
    return None, "axis %r (all elements, or the two trailing axes of (K, m, n) fields)" % (tuple(axis),)


def _counts(dev_f, dev_o, K, npix, shared, thr_f, thr_o):
    """uint64 ``(K, nthr, 4)`` of device fields: hits, misses, false alarms, correct negatives; thresholds are the
    float64 numbers to compare with."""
    tf = np.ascontiguousarray(thr_f, dtype=np.float64)
    to = np.ascontiguousarray(thr_o, dtype=np.float64)
    out = DeviceArray((K, tf.size, 4), np.uint64)
    _lib.check(
        _lib.lib().psh_detcat_counts_dev(dev_f.ptr, int(dev_f.dtype == np.float64), dev_o.ptr, int(dev_o.dtype == np.float64),
                                         int(bool(shared)), int(K), int(npix), tf.ctypes.data_as(ctypes.c_void_p),
                                         to.ctypes.data_as(ctypes.c_void_p), int(tf.size), out.ptr),
        "psh_detcat_counts_dev",
    )
    return np.array(out.to_host())  # the copy waits for the kernels: the fields may go after it


def det_cat_fct(pred, obs, thr, scores="", axis=None):
    """Calculate simple and skill scores for deterministic categorical (dichotomous) forecasts: ``pred`` and ``obs`` of
    one shape, an event is a value ``> thr``; ``scores`` names the scores (ACC, BIAS, CSI, ETS, F1, FA, FAR, GSS, HK,
    HSS, MCC, POD, SEDI; ``""``: all), ``axis`` the axes they are integrated over (None: all elements).  Returns the
    dict of results."""
    contab = det_cat_fct_init(thr, axis)
    det_cat_fct_accum(contab, pred, obs)
    return det_cat_fct_compute(contab, scores)


def det_cat_fct_init(thr, axis=None):
    """Initialize a contingency table object: the reference's dict, ``axis`` stored as the reference stores it (None, the
    iterable itself, or a one-element tuple)."""
    return {"thr": thr, "axis": _as_iterable_axis(axis), "hits": None, "false_alarms": None, "misses": None,
            "correct_negatives": None}


def det_cat_fct_accum(contab, pred, obs):
    """Accumulate the frequency of "yes" and "no" forecasts and observations of ``pred`` and ``obs`` (NumPy or
    DeviceArray) in the contingency table ``contab`` made by :func:`det_cat_fct_init` (or by the reference's)."""
    resident = isinstance(pred, DeviceArray) or isinstance(obs, DeviceArray)
    axis = _check_fields(pred, obs, contab["axis"])
    dt_f, dt_o = _dtype_of(pred), _dtype_of(obs)
    layout, why = _layout(tuple(pred.shape), axis, (dt_f, dt_o))
    if why is not None:
        return decline("det_cat_fct_accum", why, lookup("verification.detcatscores", "det_cat_fct_accum", det_cat_fct_accum),
                       resident)(contab, pred, obs)
    K, npix, nshape = layout
    if contab["hits"] is None:
        for key in _COUNT_KEYS:
            contab[key] = np.zeros(nshape, dtype=int)
    elif contab["hits"].shape != nshape:
        raise ValueError("the shape of the input arrays does not match the shape of the contingency table %s!=%s"
                         % (nshape, contab["hits"].shape))
    thr = contab["thr"]
    counts = _counts(_upload(pred), _upload(obs), K, npix, False, [_compared_as(thr, dt_f)], [_compared_as(thr, dt_o)])
    for c, key in enumerate(_COUNT_KEYS):
        contab[key] += counts[:, 0, c].astype(int).reshape(nshape)


def det_cat_fct_merge(contab_1, contab_2):
    """Merge two contingency table objects; returns the merged object (it shares its arrays with ``contab_1``, as in the
    reference)."""
    if contab_1["thr"] != contab_2["thr"]:
        raise ValueError("cannot merge: the thresholds are not same %s!=%s" % (contab_1["thr"], contab_2["thr"]))
    if contab_1["axis"] != contab_2["axis"]:
        raise ValueError("cannot merge: the axis are not same %s!=%s" % (contab_1["axis"], contab_2["axis"]))
    if contab_1["hits"] is None or contab_2["hits"] is None:
        raise ValueError("cannot merge: no data found")
    contab = contab_1.copy()
    contab["hits"] += contab_2["hits"]
    contab["misses"] += contab_2["misses"]
    contab["false_alarms"] += contab_2["false_alarms"]
    contab["correct_negatives"] += contab_2["correct_negatives"]
    return contab


def det_cat_fct_compute(contab, scores=""):
    """Compute the scores named by ``scores`` (see :func:`det_cat_fct`) from a contingency table object; every
    operation in the reference's order, so that the results - the NaN and inf of an empty margin and NumPy's warnings
    with them - are the reference's."""
    H = 1.0 * contab["hits"]
    M = 1.0 * contab["misses"]
    F = 1.0 * contab["false_alarms"]
    R = 1.0 * contab["correct_negatives"]
    result = {}
    for score in _as_iterable_scores(scores):
        if score is None:
            continue
        name = score.lower()
        POD = H / (H + M)
        FAR = F / (H + F)
        FA = F / (F + R)
        s = (H + M) / (H + M + F + R)
        if name in ("pod", ""):
            result["POD"] = POD
        if name in ("far", ""):
            result["FAR"] = FAR
        if name in ("fa", ""):
            result["FA"] = FA
        if name in ("acc", ""):
            result["ACC"] = (H + R) / (H + M + F + R)
        if name in ("csi", ""):
            result["CSI"] = H / (H + M + F)
        if name in ("bias", ""):
            result["BIAS"] = (H + F) / (H + M)
        if name in ("hss", ""):
            result["HSS"] = 2 * (H * R - F * M) / ((H + M) * (M + R) + (H + F) * (F + R))
        if name in ("hk", ""):
            result["HK"] = POD - FA
        if name in ("gss", "ets", ""):
            GSS = (POD - FA) / ((1 - s * POD) / (1 - s) + FA * (1 - s) / s)
            result["ETS" if name == "ets" else "GSS"] = GSS
        if name in ("sedi", ""):
            result["SEDI"] = (np.log(FA) - np.log(POD) + np.log(1 - POD) - np.log(1 - FA)) / (
                np.log(FA) + np.log(POD) + np.log(1 - POD) + np.log(1 - FA))
        if name in ("mcc", ""):
            result["MCC"] = (H * R - F * M) / np.sqrt((H + F) * (H + M) * (R + F) * (R + M))
        if name in ("f1", ""):
            result["F1"] = 2 * H / (2 * H + F + M)
    return result


def _table_fields(name, X_f, X_o):
    """``(K, npix, shared, single)`` of a stack ``(K, m, n)`` or one field ``(m, n)`` against a plane or a matching
    stack."""
    shape_f, shape_o = tuple(X_f.shape), tuple(X_o.shape)
    single = len(shape_f) == 2
    if single:
        shape_f = (1,) + shape_f
    if len(shape_f) != 3 or shape_o not in (shape_f, shape_f[1:]):
        raise ValueError("X_f must have shape (m, n) or (K, m, n) and X_o shape (m, n) or that of X_f")
    for dtype in (_dtype_of(X_f), _dtype_of(X_o)):
        if dtype not in _NATIVE:
            raise NotImplementedError("pysteps_amd %s: dtype %s is not implemented on the device" % (name, dtype))
    K, m, n = shape_f
    if m * n < 1:
        raise ValueError("%s: empty fields" % name)
    return K, m * n, len(shape_o) == 2 or K == 1, single


def _table_counts(X_f, X_o, thrs, widen):
    """uint64 ``(K, nthr, 4)``; ``widen``: float32 forecasts are compared as their float64 values."""
    K, npix, shared, _ = _table_fields("det_cat_table", X_f, X_o)
    dt_f, dt_o = _dtype_of(X_f), _dtype_of(X_o)
    as_f = np.dtype(np.float64) if widen else dt_f
    return _counts(_upload(X_f), _upload(X_o), K, npix, shared, [_compared_as(t, as_f) for t in thrs],
                   [_compared_as(t, dt_o) for t in thrs])


def _table_object(counts):
    """A contingency table object (without threshold and axis) whose arrays have the leading shape of ``counts``."""
    return {key: counts[..., c].astype(int) for c, key in enumerate(_COUNT_KEYS)}


def det_cat_table(X_f, X_o, thrs, return_counts=False, scores=""):
    """The categorical scores of every forecast of ``X_f`` - ``(K, m, n)``, or one field ``(m, n)`` - against ``X_o`` -
    one observation ``(m, n)`` shared by all of them, or a stack like ``X_f`` - for every threshold of ``thrs``, in one
    call: the dict of :func:`det_cat_fct` with float64 arrays ``(K, nthr)``, or ``(nthr,)`` for a single field, each
    entry equal to ``det_cat_fct(X_f[k], X_o, thr)``.  ``return_counts=True`` returns ``(scores, counts)``, ``counts``
    the integers ``(..., 4)`` uint64: hits, misses, false alarms, correct negatives.  NumPy or DeviceArray fields,
    float32 or float64."""
    thrs = [thrs] if np.isscalar(thrs) else list(thrs)
    if not thrs:
        raise ValueError("det_cat_table: no threshold given")
    counts = _table_counts(X_f, X_o, thrs, False)
    if len(X_f.shape) == 2:
        counts = counts[0]
    result = det_cat_fct_compute(_table_object(counts), scores)
    return (result, counts) if return_counts else result
