"""Ensemble skill and spread on the device, mirror of ``pysteps.verification.ensscores`` ``ensemble_skill`` and
``ensemble_spread`` (reference: pysteps/verification/ensscores.py; Zacharov and Rezacova 2009).

``ensemble_skill`` is the mean of a deterministic score of every member against one observation, ``ensemble_spread`` the
mean of the same score between all K (K - 1) / 2 pairs of members (i, j), i < j, with member i as the prediction and
member j as the observation, in the reference's loop order (i outer, j inner).  The reference indexes a score's result
dict with ``metric`` as it was given, so ``"RMSE"``, ``"CSI"`` and ``"corr_p"`` work and ``"rmse"`` raises ``KeyError``;
so do these.  The mean is ``np.mean`` over the Python list of the scores in that order, as in the reference.

How a metric is served (names as the reference's ``get_method(metric, type="deterministic")`` takes them):

* categorical names (``thr=``): ``psh_detcat_pairs_dev`` (csrc/ensscores.hip) counts the hits of every pair and the
  events of every member in one read of the stack; a pair's contingency table follows from them as exact integers and
  :func:`~pysteps_amd.verification.detcatscores.det_cat_fct_compute` gives the reference's bits.
* online continuous names without conditioning: ``psh_detcont_pairs_dev`` sums what the metric's formula reads
  (``_SUM_MASK``) for every pair, bit for bit what ``psh_detcont_sums_dev`` sums for (member i, member j); each member's
  own sums come from one call of that entry point with the stack on both sides.  Moments and scores are those of
  :mod:`~pysteps_amd.verification.detcontscores`.
* continuous names with ``conditioning`` (a member's own pixel set then depends on the pair) and ``fss``: this package's
  ``det_cont_fct`` / ``fss`` pair by pair on the planes of the stack where it lies.
* ``corr_s``, ``scatter``, ``binary_mse``, ``sal``, more than 64 members, another dtype, an infinite value under a
  continuous metric: the reference's function with a ``RuntimeWarning`` when pysteps is importable and the stack is a
  NumPy array, ``NotImplementedError`` otherwise.

``rankhist`` stays the reference's: it breaks ties with unseeded random numbers.
"""

import ctypes

import numpy as np

from .. import _lib
from .._reference import decline, lookup
from ..device import DeviceArray, _compared_as, _dtype_of, _upload
from . import detcatscores, detcontscores, spatialscores

__all__ = ["ensemble_skill", "ensemble_spread", "pair_scores", "SpreadSkillAccumulator"]

MAX_MEMBERS = 64
_CATEGORICAL = ("acc", "bias", "csi", "f1", "fa", "far", "gss", "hk", "hss", "mcc", "pod", "sedi")
_CONTINUOUS = ("beta", "beta1", "beta2", "corr_p", "corr_s", "drmse", "mae", "mse", "me", "nmse", "rmse", "rv", "scatter")
_REFERENCE_ONLY = ("corr_s", "scatter", "binary_mse", "sal")
_R = detcontscores  # the kernel's sums by number
# the pair sums (bits of psh_detcont_pairs_dev's sum_mask) behind the moments a metric's formula reads: me <- res,
# mse <- res^2, mae <- |res|, mss <- (pred + obs)^2, cov <- obs pred and each side over the pairs
_MOMENT_SUMS = {"me": (_R._RES,), "mse": (_R._RES2,), "mae": (_R._ABS,), "mss": (_R._SUM2,),
                "cov": (_R._OBS_PAIR, _R._PRED_PAIR, _R._OBS_PRED), "vobs": (), "vpred": (), "mobs": (), "mpred": ()}
_METRIC_MOMENTS = {"me": ("me",), "mae": ("mae",), "mse": ("mse",), "nmse": ("mse", "mss"), "rmse": ("mse",),
                   "corr_p": ("cov", "vobs", "vpred"), "beta": ("cov", "vpred"), "beta1": ("cov", "vpred"),
                   "beta2": ("cov", "vobs"), "drmse": ("mse", "me"), "rv": ("mse", "vobs")}
_SUM_MASK = {name: sum(1 << s for s in sorted({s for m in moments for s in _MOMENT_SUMS[m]}))
             for name, moments in _METRIC_MOMENTS.items()}
FULL_MASK = 127


def _stock(name):
    """The reference's function ``name`` of pysteps.verification.ensscores, or None when pysteps is not importable."""
    return lookup("verification.ensscores", name, globals()[name])


def _pair_table(K):
    """int32 ``(K (K - 1) / 2, 2)``: the members (i, j) of every pair in the order the kernels number them."""
    i, j = np.triu_indices(K, 1)
    return np.stack([i, j], axis=1).astype(np.int32)


def _check_stack(X_f):
    if len(X_f.shape) != 3:
        raise ValueError("the number of dimensions of X_f must be equal to 3, " + "but %i dimensions were passed" % len(X_f.shape))


def _check_members(X_f):
    if X_f.shape[0] < 2:
        raise ValueError("the number of members in X_f must be greater than 1," + " but %i members were passed" % X_f.shape[0])


def _kind(metric):
    """``(name, "categorical" | "continuous" | "fss" | "reference")`` of a metric as the reference's ``get_method``
    reads it; its ``ValueError`` for a name it does not know."""
    name = "none" if metric is None else metric.lower()
    if name in _REFERENCE_ONLY:
        return name, "reference"
    if name in _CATEGORICAL:
        return name, "categorical"
    if name in _CONTINUOUS:
        return name, "continuous"
    if name == "fss":
        return name, "fss"
    raise ValueError("unknown deterministic method %s" % name)


def _plain(kwargs):
    """The continuous metric is asked for every pixel of the planes: no conditioning, no axis, nothing else."""
    return set(kwargs) <= {"thr", "conditioning", "axis"} and kwargs.get("conditioning") is None and kwargs.get("axis") is None


def _cat_pairs(stack, K, npix, thrs):
    """``(hits (nthr, pairs), events (nthr, K))`` uint64 of a device stack; thresholds are the float64 numbers to compare
    with."""
    thr = np.ascontiguousarray(thrs, dtype=np.float64)
    npairs = K * (K - 1) // 2
    hits = DeviceArray((thr.size, npairs), np.uint64)
    events = DeviceArray((thr.size, K), np.uint64)
    _lib.check(
        _lib.lib().psh_detcat_pairs_dev(stack.ptr, int(stack.dtype == np.float64), int(K), int(npix),
                                        thr.ctypes.data_as(ctypes.c_void_p), int(thr.size), hits.ptr, events.ptr),
        "psh_detcat_pairs_dev",
    )
    return np.array(hits.to_host()), np.array(events.to_host())  # the copies wait for the kernels


def _cont_pairs(stack, K, npix, sum_mask):
    """``(counts (pairs,) uint64, sums (pairs, 7, 2) float64)`` of a device stack: the pixels of a pair whose residual
    is finite and the pair sums ``sum_mask`` selects as (hi, lo), zeros elsewhere."""
    npairs = K * (K - 1) // 2
    counts = DeviceArray((npairs,), np.uint64)
    sums = DeviceArray((npairs, 7, 2), np.float64)
    _lib.check(
        _lib.lib().psh_detcont_pairs_dev(stack.ptr, int(stack.dtype == np.float64), int(K), int(npix), int(sum_mask), counts.ptr,
                                         sums.ptr),
        "psh_detcont_pairs_dev",
    )
    return np.array(counts.to_host()), np.array(sums.to_host())


def _pair_tables(hits, events, npix, K):
    """The contingency tables of every pair - int arrays ``(pairs,)`` under the keys of a table object - from the hits
    of the pairs and the events of the members, one threshold."""
    ij = _pair_table(K)
    h = hits.astype(int)
    n_i, n_j = events.astype(int)[ij[:, 0]], events.astype(int)[ij[:, 1]]
    return {"hits": h, "false_alarms": n_i - h, "misses": n_j - h, "correct_negatives": int(npix) - n_i - n_j + h}


def _pair_sums(pair_counts, pair_sums, own_counts, own_sums, K):
    """``(counts (pairs, 4), sums (pairs, 11, 2))`` as ``psh_detcont_sums_dev`` lays them out for (member i, member j):
    the pair kernel's seven sums, then member j's own as the observation and member i's own as the prediction."""
    ij = _pair_table(K)
    counts = np.zeros((ij.shape[0], 4), dtype=np.uint64)
    counts[:, 0] = own_counts[ij[:, 1], 0]
    counts[:, 1] = own_counts[ij[:, 0], 1]
    counts[:, 2] = pair_counts
    sums = np.zeros((ij.shape[0], 11, 2), dtype=np.float64)
    sums[:, :7] = pair_sums
    sums[:, [_R._OBS, _R._OBS2]] = own_sums[ij[:, 1]][:, [_R._OBS, _R._OBS2]]
    sums[:, [_R._PRED, _R._PRED2]] = own_sums[ij[:, 0]][:, [_R._PRED, _R._PRED2]]
    return counts, sums


def _own(stack, K, npix):
    """Every member's own counts and sums: the stack against itself, member by member, without conditioning."""
    return detcontscores._sums(stack, stack, K, npix, False, 0, 0.0, 0.0)


def _declined(X_f, name, kind):
    """Why the device path declines this stack for this metric, or None."""
    if kind == "reference":
        return "the metric %s" % name
    if X_f.shape[0] > MAX_MEMBERS:
        return "%d members (at most %d)" % (X_f.shape[0], MAX_MEMBERS)
    if _dtype_of(X_f) not in detcatscores._NATIVE:
        return "dtype %s" % _dtype_of(X_f)
    if int(np.prod(X_f.shape[1:], dtype=np.int64)) < 1:
        return "an empty field"
    return None


def _pair_values(X_f, metric, kwargs):
    """The list of the scores of all pairs in the reference's order, or the reason why the device path declines."""
    name, kind = _kind(metric)
    why = _declined(X_f, name, kind)
    if why is not None:
        return None, why
    K, npix = X_f.shape[0], int(X_f.shape[1]) * int(X_f.shape[2])
    dtype = _dtype_of(X_f)
    stack = _upload(X_f)
    if kind == "categorical":
        kwargs = dict(kwargs)
        thr = kwargs.pop("thr")
        hits, events = _cat_pairs(stack, K, npix, [_compared_as(thr, dtype)])
        result = detcatscores.det_cat_fct_compute(_pair_tables(hits[0], events[0], npix, K), [name])
        return list(result[metric]), None
    if kind == "continuous":
        own_counts, own_sums = _own(stack, K, npix)
        if own_counts[:, 3].any():
            return None, "an infinite value"
        if _plain(kwargs):
            pair_counts, pair_sums = _cont_pairs(stack, K, npix, _SUM_MASK[name])
            counts, sums = _pair_sums(pair_counts, pair_sums, own_counts, own_sums, K)
            err = detcontscores.det_cont_fct_init(thr=kwargs.get("thr", 0.0))
            detcontscores._zeros(err, (counts.shape[0],))
            batch, n = detcontscores._batch(counts, sums, (counts.shape[0],))
            detcontscores._merge_into(err, batch, n)
            return list(detcontscores.det_cont_fct_compute(err, [name])[metric]), None
        call = lambda a, b: detcontscores.det_cont_fct(a, b, [name], **kwargs)  # noqa: E731
    else:
        call = lambda a, b: spatialscores.fss(a, b, **kwargs)  # noqa: E731
    values = []
    for i, j in _pair_table(K):
        value = call(stack.view(int(i)), stack.view(int(j)))
        values.append(value[metric] if isinstance(value, dict) else value)
    return values, None


def pair_scores(X_f, metric, **kwargs):
    """The score ``metric`` between all pairs of the members of ``X_f`` ``(K, m, n)``, NumPy or DeviceArray: float64
    ``(K, K)`` with entry ``[i, j]``, ``i < j``, the score of member i as the prediction against member j as the
    observation, NaN elsewhere.  :func:`ensemble_spread` is the mean of the entries in row-major order.  A stack or a
    metric the device path declines raises ``NotImplementedError``."""
    _check_stack(X_f)
    _check_members(X_f)
    values, why = _pair_values(X_f, metric, kwargs)
    if why is not None:
        raise NotImplementedError("pysteps_amd pair_scores: %s is not implemented on the device" % why)
    K = X_f.shape[0]
    out = np.full((K, K), np.nan, dtype=np.float64)
    out[np.triu_indices(K, 1)] = np.asarray(values, dtype=np.float64)
    return out


def ensemble_skill(X_f, X_o, metric, **kwargs):
    """Compute mean ensemble skill for a given skill metric: the mean over the members of ``X_f`` ``(l, m, n)`` of the
    deterministic score ``metric`` against the observed field ``X_o`` ``(m, n)``; ``kwargs`` are the score's own
    (``thr=`` for a categorical one, ``thr=`` and ``scale=`` for ``"fss"``)."""
    _check_stack(X_f)
    if tuple(X_f.shape[1:]) != tuple(X_o.shape):
        raise ValueError("the shape of X_f does not match the shape of " + "X_o (%d,%d)!=(%d,%d)"
                         % (X_f.shape[1], X_f.shape[2], X_o.shape[0], X_o.shape[1]))
    name, kind = _kind(metric)
    resident = isinstance(X_f, DeviceArray) or isinstance(X_o, DeviceArray)
    why = _declined(X_f, name, kind)
    if why is None and _dtype_of(X_o) not in detcatscores._NATIVE:
        why = "dtype %s" % _dtype_of(X_o)
    if why is None:
        try:
            if kind == "categorical":
                kwargs = dict(kwargs)
                skill = detcatscores.det_cat_table(X_f, X_o, [kwargs.pop("thr")], scores=[name])[metric][:, 0]
            elif kind == "continuous" and _plain(kwargs):
                skill = detcontscores.det_cont_table(X_f, X_o, thr=kwargs.get("thr", 0.0), scores=[name])[metric]
            elif kind == "continuous" and set(kwargs) <= {"thr", "conditioning"}:
                skill = detcontscores.det_cont_table(X_f, X_o, kwargs["conditioning"], kwargs.get("thr", 0.0), scores=[name])[metric]
            elif kind == "fss" and set(kwargs) == {"thr", "scale"}:
                skill = spatialscores.fss_table(X_f, X_o, [kwargs["thr"]], [kwargs["scale"]])[:, 0, 0]
            else:  # the score's own signature decides about these keywords, member by member
                stack, obs = _upload(X_f), _upload(X_o)
                skill = []
                for k in range(X_f.shape[0]):
                    value = (spatialscores.fss(stack.view(k), obs, **kwargs) if kind == "fss"
                             else detcontscores.det_cont_fct(stack.view(k), obs, [name], **kwargs))
                    skill.append(value[metric] if isinstance(value, dict) else value)
            return np.mean(list(skill))
        except NotImplementedError as exc:  # an infinite value, a scale or a threshold the table kernels decline
            why = str(exc).split(": ", 1)[-1].replace(" is not implemented on the device", "")
    return decline("ensemble_skill", why, _stock("ensemble_skill"), resident)(X_f, X_o, metric, **kwargs)


def ensemble_spread(X_f, metric, **kwargs):
    """Compute mean ensemble spread for a given skill metric: the mean of the deterministic score ``metric`` between
    all possible pairs of the members of ``X_f`` ``(l, m, n)``; ``kwargs`` are the score's own."""
    _check_stack(X_f)
    _check_members(X_f)
    try:
        values, why = _pair_values(X_f, metric, kwargs)
    except NotImplementedError as exc:
        values, why = None, str(exc).split(": ", 1)[-1].replace(" is not implemented on the device", "")
    if why is not None:
        return decline("ensemble_spread", why, _stock("ensemble_spread"), isinstance(X_f, DeviceArray))(X_f, metric, **kwargs)
    return np.mean(values)


class SpreadSkillAccumulator:
    """Ensemble skill and spread of a nowcast per lead time, usable as the ``callback`` of a nowcast::

        acc = SpreadSkillAccumulator(observations, ["CSI", "RMSE"], thr=1.0)
        nowcasts.get_method("steps")(..., callback=acc, return_output=False)
        acc.skill, acc.spread      # (n_leadtimes, n_metrics)

    ``observations`` is ``(n_leadtimes, m, n)``, NumPy or DeviceArray, and is kept on the device.  Call ``t`` receives
    the members of lead time ``t`` - a ``DeviceArray`` ``(k, m, n)`` from the resident nowcast loop, a host ``ndarray``
    from any other - and records :func:`ensemble_skill` against ``observations[t]`` and :func:`ensemble_spread` for every
    metric of ``metrics`` (names as the two functions take them).  ``thr`` is handed to the categorical metrics."""

    accepts_device = True

    def __init__(self, observations, metrics, thr=None):
        self.metrics = [metrics] if isinstance(metrics, str) else list(metrics)
        if not self.metrics:
            raise ValueError("SpreadSkillAccumulator: no metric given")
        for metric in self.metrics:
            if _kind(metric)[1] not in ("categorical", "continuous"):
                raise ValueError("SpreadSkillAccumulator: %s is not a categorical or continuous metric" % metric)
            if _kind(metric)[1] == "categorical" and thr is None:
                raise ValueError("SpreadSkillAccumulator: the categorical metric %s needs thr" % metric)
        if len(observations.shape) != 3:
            raise ValueError("SpreadSkillAccumulator: observations of shape (n_leadtimes, m, n) expected, got %s"
                             % (tuple(observations.shape),))
        self._obs = observations if isinstance(observations, DeviceArray) else DeviceArray.from_host(np.asarray(observations))
        self.thr = thr
        self._skill, self._spread = [], []
        self.n_leadtimes = 0
        self.received = []  # type of the members of every call: DeviceArray or ndarray

    def __call__(self, members):
        resident = isinstance(members, DeviceArray)
        self.received.append(DeviceArray if resident else np.ndarray)
        if len(members.shape) != 3 or tuple(members.shape[1:]) != self._obs.shape[1:]:
            raise ValueError("SpreadSkillAccumulator: members of shape (k, %d, %d) expected, got %s"
                             % (self._obs.shape[1:] + (tuple(members.shape),)))
        if self.n_leadtimes >= self._obs.shape[0]:
            raise ValueError("SpreadSkillAccumulator: called for more lead times than the %d observations" % self._obs.shape[0])
        obs = self._obs.view(self.n_leadtimes)
        stack = members if resident else np.asarray(members)  # a host stack keeps the way to the reference open
        skill, spread = [], []
        with np.errstate(all="ignore"):
            for metric in self.metrics:
                kwargs = {"thr": self.thr} if _kind(metric)[1] == "categorical" else {}
                skill.append(ensemble_skill(stack, obs, metric, **kwargs))
                spread.append(ensemble_spread(stack, metric, **kwargs))
        self._skill.append(skill)
        self._spread.append(spread)
        self.n_leadtimes += 1

    @property
    def skill(self):
        """float64 ``(n_leadtimes, n_metrics)``: :func:`ensemble_skill` per lead time and metric."""
        return np.array(self._skill, dtype=np.float64).reshape(self.n_leadtimes, len(self.metrics))

    @property
    def spread(self):
        """float64 ``(n_leadtimes, n_metrics)``: :func:`ensemble_spread` per lead time and metric."""
        return np.array(self._spread, dtype=np.float64).reshape(self.n_leadtimes, len(self.metrics))
