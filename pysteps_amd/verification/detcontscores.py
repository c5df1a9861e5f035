"""Deterministic continuous scores on the device, mirror of ``pysteps.verification.detcontscores`` ``det_cont_fct``,
``det_cont_fct_init``, ``det_cont_fct_accum``, ``det_cont_fct_merge`` and ``det_cont_fct_compute`` (reference:
pysteps/verification/detcontscores.py).

What the reference's ``det_cont_fct_accum`` adds to the verification error object, as its code (not its docstring) has
it: ``n`` counts the pairs whose residual ``pred - obs`` is finite; ``me``, ``mse``, ``mss`` and ``mae`` are the means
of the residual, its square, ``(pred + obs)**2`` and its absolute value over those pairs; ``mobs`` and ``mpred`` are
the means of each field over its own finite pixels; ``vobs`` and ``vpred`` the mean squared deviations from those means
over each field's finite pixels and ``cov`` the mean product of the deviations over the pairs.  Conditioning
(``"single"``: either side ``> thr``, ``"double"``: both) turns the excluded pixels into NaN on both sides first.  All
nine are then merged into the object with ``n`` as the weight.

``psh_detcont_sums_dev`` (csrc/detscores.hip) reads the fields once and returns the three counts and eleven raw sums
as double-double pairs; :func:`det_cont_fct_accum` forms the nine batch quantities from them in exact rational
arithmetic, rounds each once to float64 and applies the reference's merge formulas.  ``_merge`` and ``_compute`` are
host arithmetic on a handful of numbers, restated operation by operation.  For float32 fields the reference forms
residuals, squares and means in float32; the device widens first and is the more exact side
(tests/test_detscores_cpu.py measures the reference's deviation from the definitions above).

Served on the device: ``axis=None`` and the two trailing axes of ``(K, m, n)`` fields, float32 or float64 on either
side, finite or NaN values.  Any other axis (the negative ones mean "no integration" in the reference), another dtype or
an infinite value goes to the reference's function with a ``RuntimeWarning`` when pysteps is importable and the fields
are NumPy arrays, and raises ``NotImplementedError`` otherwise.  The offline scores ``corr_s`` and ``scatter`` of
:func:`det_cont_fct` (``scores=""`` asks for them too) are the reference's in the same way; the online scores of the same
call still come from the device.  Like the reference's, ``det_cont_fct_merge`` copies the dict of its first argument,
not its arrays.
"""

import ctypes
import warnings
from fractions import Fraction

import numpy as np

from .. import _lib
from .._reference import decline, lookup
from ..device import DeviceArray, _compared_as, _dtype_of, _upload
from .detcatscores import _as_iterable_axis, _as_iterable_scores, _check_fields, _layout, _table_fields

__all__ = ["det_cont_fct", "det_cont_fct_init", "det_cont_fct_accum", "det_cont_fct_merge", "det_cont_fct_compute",
           "det_cont_table"]

_MOMENT_KEYS = ("cov", "vobs", "vpred", "mobs", "mpred", "me", "mse", "mss", "mae")
_OFFLINE = ("scatter", "corr_s")
# the kernel's sums (csrc/detscores.hip): over the pairs, then over each field's finite pixels
_RES, _RES2, _ABS, _SUM2, _OBS_PAIR, _PRED_PAIR, _OBS_PRED, _OBS, _OBS2, _PRED, _PRED2 = range(11)
_CONDITIONING = {None: 0, "single": 1, "double": 2}


def _stock(name):
    """The reference's function ``name`` of pysteps.verification.detcontscores, or None when pysteps is not importable."""
    return lookup("verification.detcontscores", name, globals()[name])


def _conditioning_code(conditioning):
    try:
        return _CONDITIONING[conditioning]
    except (KeyError, TypeError):
        raise ValueError("unkown conditioning %s" % conditioning) from None


def _sums(dev_f, dev_o, K, npix, shared, conditioning, thr_f, thr_o):
    """``(counts (K, 4) uint64, sums (K, 11, 2) float64)`` of device fields: finite observations, finite predictions,
    finite pairs and infinite values; the raw sums as (hi, lo) pairs.  ``conditioning`` is the kernel's code, the
    thresholds the float64 numbers to compare with."""
    counts = DeviceArray((K, 4), np.uint64)
    sums = DeviceArray((K, 11, 2), np.float64)
    _lib.check(
        _lib.lib().psh_detcont_sums_dev(dev_f.ptr, int(dev_f.dtype == np.float64), dev_o.ptr, int(dev_o.dtype == np.float64),
                                        int(bool(shared)), int(K), int(npix), int(conditioning), float(thr_f), float(thr_o),
                                        counts.ptr, sums.ptr),
        "psh_detcont_sums_dev",
    )
    return np.array(counts.to_host()), np.array(sums.to_host())  # the copies wait for the kernels


def _moments(counts, sums):
    """The nine batch quantities of one forecast and its pair count from the kernel's counts and double-double sums:
    exact rational arithmetic, one rounding to float64 each.  NaN where the reference takes the mean of nothing."""
    n_obs, n_pred, n = int(counts[0]), int(counts[1]), int(counts[2])
    S = [Fraction(float(hi)) + Fraction(float(lo)) for hi, lo in sums]
    out = dict.fromkeys(_MOMENT_KEYS, np.float64(np.nan))
    mobs = S[_OBS] / n_obs if n_obs else None
    mpred = S[_PRED] / n_pred if n_pred else None
    if mobs is not None:
        out["mobs"] = np.float64(float(mobs))
        out["vobs"] = np.float64(float(S[_OBS2] / n_obs - mobs * mobs))
    if mpred is not None:
        out["mpred"] = np.float64(float(mpred))
        out["vpred"] = np.float64(float(S[_PRED2] / n_pred - mpred * mpred))
    if n:
        out["me"] = np.float64(float(S[_RES] / n))
        out["mse"] = np.float64(float(S[_RES2] / n))
        out["mss"] = np.float64(float(S[_SUM2] / n))
        out["mae"] = np.float64(float(S[_ABS] / n))
        # mean of (obs - mobs) (pred - mpred) over the pairs, the means those of each field on its own
        out["cov"] = np.float64(float((S[_OBS_PRED] - mobs * S[_PRED_PAIR] - mpred * S[_OBS_PAIR]) / n + mobs * mpred))
    return out, n


def _batch(counts, sums, nshape):
    """Arrays of shape ``nshape`` of the batch quantities of every forecast, and the pair counts as int64."""
    per_member = [_moments(c, s) for c, s in zip(counts, sums)]
    batch = {key: np.array([m[key] for m, _ in per_member], dtype=np.float64).reshape(nshape) for key in _MOMENT_KEYS}
    return batch, np.array([n for _, n in per_member], dtype=np.int64).reshape(nshape)


def _merge_mean(avg_a, count_a, avg_b, count_b):
    sel = count_b > 0
    avg_a[sel] = (count_a[sel] * avg_a[sel] + count_b[sel] * avg_b[sel]) / (count_a[sel] + count_b[sel])


def _merge_var(avg_a, count_a, var_a, avg_b, count_b, var_b):
    sel = count_b > 0
    delta = avg_b - avg_a
    m_a = var_a * count_a
    m_b = var_b * count_b
    var_a[sel] = m_a[sel] + m_b[sel] + delta[sel] ** 2 * count_a[sel] * count_b[sel] / (count_a[sel] + count_b[sel])
    var_a[sel] = var_a[sel] / (count_a[sel] + count_b[sel])


def _merge_cov(cov_a, avg_xa, avg_ya, count_a, cov_b, avg_xb, avg_yb, count_b):
    sel = count_b > 0
    deltax = avg_xb - avg_xa
    deltay = avg_yb - avg_ya
    c_a = cov_a * count_a
    c_b = cov_b * count_b
    cov_a[sel] = c_a[sel] + c_b[sel] + deltax[sel] * deltay[sel] * count_a[sel] * count_b[sel] / (count_a[sel] + count_b[sel])
    cov_a[sel] = cov_a[sel] / (count_a[sel] + count_b[sel])


def _merge_into(err, other, n):
    """Update the arrays of ``err`` in place with the moments ``other`` of ``n`` pairs: variances and covariance first
    (they need the means as they were), then the means, then the count - the reference's order."""
    _merge_var(err["mobs"], err["n"], err["vobs"], other["mobs"], n, other["vobs"])
    _merge_var(err["mpred"], err["n"], err["vpred"], other["mpred"], n, other["vpred"])
    _merge_cov(err["cov"], err["mobs"], err["mpred"], err["n"], other["cov"], other["mobs"], other["mpred"], n)
    for key in ("mobs", "mpred", "me", "mse", "mss", "mae"):
        _merge_mean(err[key], err["n"], other[key], n)
    err["n"] += n


def _zeros(err, nshape):
    for key in _MOMENT_KEYS + ("n",):
        err[key] = np.zeros(nshape)


def det_cont_fct(pred, obs, scores="", axis=None, conditioning=None, thr=0.0):
    """Calculate simple and skill scores for deterministic continuous forecasts: ``scores`` names them (beta1, beta2,
    corr_p, corr_s*, DRMSE, MAE, ME, MSE, NMSE, RMSE, RV, scatter*; ``""``: all), ``axis`` the axes they are
    integrated over (None: all elements), ``conditioning`` / ``thr`` the pairs that take part (see the module
    docstring).  The scores marked * cannot be accumulated: they are the reference's own, computed on the host.
    Returns the dict of results."""
    scores = _as_iterable_scores(scores)
    online, offline = [], []
    for score in scores:
        is_offline = str(score).lower() in _OFFLINE
        if (not is_offline or score == "") and score not in online:
            online.append(score)
        if (is_offline or score == "") and score not in offline:
            offline.append(score)
    result = {}
    if online:
        err = det_cont_fct_init(axis=axis, conditioning=conditioning, thr=thr)
        det_cont_fct_accum(err, pred, obs)
        result = det_cont_fct_compute(err, online)
    names = [name for name in ("corr_s", "scatter") if "" in offline or name in [str(s).lower() for s in offline]]
    if names:
        resident = isinstance(pred, DeviceArray) or isinstance(obs, DeviceArray)
        ref = decline("det_cont_fct", "the offline score%s %s" % ("s" if len(names) > 1 else "", " and ".join(names)),
                       _stock("det_cont_fct"), resident)
        result.update(ref(pred, obs, scores=names, axis=axis, conditioning=conditioning, thr=thr))
    return result


def det_cont_fct_init(axis=None, conditioning=None, thr=0.0):
    """Initialize a verification error object: the reference's dict, ``axis`` stored as the reference stores it."""
    err = {"axis": _as_iterable_axis(axis), "conditioning": conditioning, "thr": thr}
    for key in _MOMENT_KEYS + ("n",):
        err[key] = None
    return err


def det_cont_fct_accum(err, pred, obs):
    """Accumulate the forecast error of ``pred`` against ``obs`` (NumPy or DeviceArray) in the verification error
    object ``err`` made by :func:`det_cont_fct_init` (or by the reference's)."""
    resident = isinstance(pred, DeviceArray) or isinstance(obs, DeviceArray)
    axis = _check_fields(pred, obs, err["axis"])
    dt_f, dt_o = _dtype_of(pred), _dtype_of(obs)
    layout, why = _layout(tuple(pred.shape), axis, (dt_f, dt_o))
    if why is not None:
        return decline("det_cont_fct_accum", why, _stock("det_cont_fct_accum"), resident)(err, pred, obs)
    K, npix, nshape = layout
    if err["cov"] is not None and err["cov"].shape != nshape:
        raise ValueError("the shape of the input arrays does not match the shape of the verification object %s!=%s"
                         % (nshape, err["cov"].shape))
    code = _conditioning_code(err["conditioning"])
    counts, sums = _sums(_upload(pred), _upload(obs), K, npix, False, code, _compared_as(err["thr"], dt_f),
                         _compared_as(err["thr"], dt_o))
    if counts[:, 3].any():
        return decline("det_cont_fct_accum", "an infinite value", _stock("det_cont_fct_accum"), resident)(err, pred, obs)
    if err["cov"] is None:
        _zeros(err, nshape)
    batch, n = _batch(counts, sums, nshape)
    if not n.all():
        warnings.warn("Mean of empty slice", RuntimeWarning, stacklevel=2)  # what the reference's nanmean says
    _merge_into(err, batch, n)


def det_cont_fct_merge(err_1, err_2):
    """Merge two verification error objects; returns the merged object (it shares its arrays with ``err_1``, as in the
    reference)."""
    if err_1["axis"] != err_2["axis"]:
        raise ValueError("cannot merge: the axis are not same %s!=%s" % (err_1["axis"], err_2["axis"]))
    if err_1["conditioning"] != err_2["conditioning"]:
        raise ValueError("cannot merge: the conditioning is not same %s!=%s" % (err_1["conditioning"], err_2["conditioning"]))
    if err_1["thr"] != err_2["thr"]:
        raise ValueError("cannot merge: the threshold is not same %s!=%s" % (err_1["thr"], err_2["thr"]))
    if err_1["cov"] is None or err_2["cov"] is None:
        raise ValueError("cannot merge: no data found")
    err = err_1.copy()
    _merge_into(err, err_2, err_2["n"])
    return err


def det_cont_fct_compute(err, scores=""):
    """Compute the scores named by ``scores`` (beta1, beta2, corr_p, DRMSE, MAE, ME, MSE, NMSE, RMSE, RV; ``""``: all)
    from a verification error object; every operation in the reference's order, so that the results - the NaN and inf
    of a vanishing variance and NumPy's warnings with them - are the reference's."""
    result = {}
    for score in _as_iterable_scores(scores):
        if score is None:
            continue
        name = score.lower()
        if name in ("bias", "me", ""):
            result["ME"] = err["me"]
        if name in ("mae", ""):
            result["MAE"] = err["mae"]
        if name in ("mse", ""):
            result["MSE"] = err["mse"]
        if name in ("nmse", ""):
            result["NMSE"] = err["mse"] / err["mss"]
        if name in ("rmse", ""):
            result["RMSE"] = np.sqrt(err["mse"])
        if name in ("corr_p", "pearsonr", ""):
            result["corr_p"] = err["cov"] / np.sqrt(err["vobs"]) / np.sqrt(err["vpred"])
        if name in ("beta", "beta1", ""):
            result["beta1"] = err["cov"] / err["vpred"]
        if name in ("beta2", ""):
            result["beta2"] = err["cov"] / err["vobs"]
        if name in ("drmse", ""):
            result["DRMSE"] = np.sqrt(err["mse"] - err["me"] ** 2)
        if name in ("rv", "brier_score", "nse", ""):
            result["RV"] = 1.0 - err["mse"] / err["vobs"]
    return result


def _table_sums(name, X_f, X_o, conditioning, thr, widen):
    """``(counts, sums, single)`` of a stack or one field against a plane or a matching stack; ``widen``: the threshold
    meets float32 forecasts as their float64 values.  Infinite values raise: there is no object to hand on."""
    K, npix, shared, single = _table_fields(name, X_f, X_o)
    dt_f, dt_o = _dtype_of(X_f), _dtype_of(X_o)
    as_f = np.dtype(np.float64) if widen else dt_f
    counts, sums = _sums(_upload(X_f), _upload(X_o), K, npix, shared, _conditioning_code(conditioning), _compared_as(thr, as_f),
                         _compared_as(thr, dt_o))
    if counts[:, 3].any():
        raise NotImplementedError("pysteps_amd %s: an infinite value is not implemented on the device" % name)
    return counts, sums, single


def det_cont_table(X_f, X_o, conditioning=None, thr=0.0, scores="", return_object=False):
    """The continuous scores of every forecast of ``X_f`` - ``(K, m, n)``, or one field ``(m, n)`` - against ``X_o`` -
    one observation ``(m, n)`` shared by all of them, or a stack like ``X_f`` - in one call: the dict of
    :func:`det_cont_fct_compute` with float64 arrays ``(K,)``, or 0-d arrays for a single field, each entry equal to
    that of ``det_cont_fct_accum`` on ``X_f[k]`` and its observation.  ``return_object=True`` returns ``(scores, err)``,
    ``err`` the verification error object behind them.  NumPy or DeviceArray fields, float32 or float64."""
    counts, sums, single = _table_sums("det_cont_table", X_f, X_o, conditioning, thr, False)
    nshape = () if single else (counts.shape[0],)
    err = det_cont_fct_init(axis=None if single else (1, 2), conditioning=conditioning, thr=thr)
    _zeros(err, nshape)
    batch, n = _batch(counts, sums, nshape)
    _merge_into(err, batch, n)
    result = det_cont_fct_compute(err, scores)
    return (result, err) if return_object else result
