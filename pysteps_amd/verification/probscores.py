"""Probabilistic scores on the device, mirror of ``pysteps.verification.probscores``: ``CRPS``, ``reldiag`` and
``ROC_curve``, each with ``_init`` / ``_accum`` / ``_compute`` (reference: pysteps/verification/probscores.py).

What the reference's ``_accum`` functions add to their objects, as its code has it:

* ``CRPS_accum`` takes the pixels where all ``k`` members and the observation are finite, sorts the members of each and
  adds Hersbach's decomposition of the CRPS, bin by bin with strict inequalities: an observation equal to a member
  adds nothing from the bins it touches.  ``psh_crps_sums_dev`` (csrc/probscores.hip) returns the number of those
  pixels and the sum as a double-double pair; differences are formed in float64 from the widened values and the
  weights ``(i/k)**2`` and ``((k-i)/k)**2`` come from :func:`crps_weights`, so ``1 - p`` is never formed from a rounded
  ``p``.  For float32 members the reference subtracts in float32; the device is the more exact side.
* ``reldiag_accum`` bins the probabilities of the pixels where probability and observation are finite with
  ``numpy.digitize(P_f, bin_edges, right=True)`` and adds, for every bin with at least ``min_count`` pixels in THIS
  call, the sum of the probabilities, the number of pixels with ``X_o >= X_min`` and the number of pixels.
* ``ROC_curve_accum`` counts, over the same pixels and for every probability threshold, hits (``P_f >= p`` and ``X_o >=
  X_min``), misses, false alarms and correct negatives.

``psh_probbins_dev`` serves the last two from one read; the object's own ``bin_edges`` and ``prob_thrs`` are compared
as they are, so objects made by the reference's ``_init`` functions and by these are interchangeable.  ``X_min`` meets
the observation and a probability threshold meets the probabilities as NumPy compares them
(``device.py::_compared_as``).  The ``_compute`` functions are host arithmetic on a handful of
numbers, restated operation by operation.  The inputs are not modified.

More than 64 members, more than 64 bins or probability thresholds, bin edges that do not increase and dtypes other
than float32 / float64 go to the reference's function with a ``RuntimeWarning`` when pysteps is importable and the
fields are NumPy arrays, and raise ``NotImplementedError`` otherwise.  :func:`crps_table` scores one member stack
against several observations, or several stacks, in one call.

``ensscores.rankhist`` has no device version on purpose: the reference breaks ties with unseeded
``np.random.uniform`` (ensscores.py:245) and precipitation ensembles are mostly ties, so its result is not a function
of its input.
"""

import ctypes

import numpy as np

from .. import _lib
from .._reference import decline, lookup
from ..device import DeviceArray, _compared_as, _dtype_of, _upload
from .detcatscores import _NATIVE

__all__ = ["CRPS", "CRPS_init", "CRPS_accum", "CRPS_compute", "reldiag", "reldiag_init", "reldiag_accum", "reldiag_compute",
           "ROC_curve", "ROC_curve_init", "ROC_curve_accum", "ROC_curve_compute", "crps_table", "crps_weights"]

MAX_MEMBERS = 64  # csrc/probscores.hip kCrpsMaxMembers
MAX_BINS = 64  # kBinsLanes: bins and probability thresholds of one pass
SWAPPED = ("CRPS", "CRPS_accum", "reldiag", "reldiag_accum", "ROC_curve", "ROC_curve_accum")


def _stock(name):
    """The reference's function ``name`` of pysteps.verification.probscores, or None when pysteps is not importable."""
    return lookup("verification.probscores", name, globals()[name])


def crps_weights(k):
    """float64 ``(k + 1, 2)``: ``(i/k)**2`` and ``((k-i)/k)**2``, one division and one product each."""
    i = np.arange(k + 1, dtype=np.float64)
    p, q = i / k, (k - i) / k
    return np.ascontiguousarray(np.stack([p * p, q * q], axis=1))


def _crps_sums(dev_f, dev_o, planes, k, npix, shared):
    """``(counts (planes,) uint64, sums (planes, 2) float64)``: the pixels that take part and the sum of their CRPS as
    (hi, lo), observation plane t against the one stack (``shared``) or against stack t."""
    counts = DeviceArray((planes,), np.uint64)
    sums = DeviceArray((planes, 2), np.float64)
    weights = crps_weights(k)
    _lib.check(
        _lib.lib().psh_crps_sums_dev(dev_f.ptr, int(dev_f.dtype == np.float64), int(bool(shared)), dev_o.ptr,
                                     int(dev_o.dtype == np.float64), int(planes), int(k), int(npix),
                                     weights.ctypes.data_as(ctypes.c_void_p), counts.ptr, sums.ptr),
        "psh_crps_sums_dev",
    )
    return np.array(counts.to_host()), np.array(sums.to_host())  # the copies wait for the kernels


def _bins(dev_p, dev_o, npix, x_min, edges, prob_thrs):
    """``(bins (n_bins, 2) uint64, sums (n_bins, 2) float64, roc (n_thrs, 4) uint64)`` of a device probability plane and
    its observation; ``edges`` / ``prob_thrs`` float64 arrays or None (its outputs are then None)."""
    n_edges = 0 if edges is None else int(edges.size)
    n_thrs = 0 if prob_thrs is None else int(prob_thrs.size)
    bins = DeviceArray((n_edges - 1, 2), np.uint64) if n_edges else None
    sums = DeviceArray((n_edges - 1, 2), np.float64) if n_edges else None
    roc = DeviceArray((n_thrs, 4), np.uint64) if n_thrs else None
    _lib.check(
        _lib.lib().psh_probbins_dev(dev_p.ptr, int(dev_p.dtype == np.float64), dev_o.ptr, int(dev_o.dtype == np.float64),
                                    int(npix), float(x_min), edges.ctypes.data_as(ctypes.c_void_p) if n_edges else None, n_edges,
                                    prob_thrs.ctypes.data_as(ctypes.c_void_p) if n_thrs else None, n_thrs,
                                    bins.ptr if n_edges else None, sums.ptr if n_edges else None, roc.ptr if n_thrs else None),
        "psh_probbins_dev",
    )
    return tuple(None if out is None else np.array(out.to_host()) for out in (bins, sums, roc))


def _size(shape):
    return int(np.prod(shape, dtype=np.int64))


# ---- CRPS ----------------------------------------------------------------------------------------------------------
def CRPS(X_f, X_o):
    """The continuous ranked probability score of the ensemble ``X_f`` ``(k, m, n, ...)`` against the observation
    ``X_o`` ``(m, n, ...)`` (NumPy or DeviceArray): a float."""
    crps = CRPS_init()
    CRPS_accum(crps, X_f, X_o)
    return CRPS_compute(crps)


def CRPS_init():
    """Initialize a CRPS object: the reference's dict."""
    return {"CRPS_sum": 0.0, "n": 0.0}


def _crps_declined(k, dtypes):
    for dtype in dtypes:
        if dtype not in _NATIVE:
            return "dtype %s" % dtype
    if k > MAX_MEMBERS:
        return "%d members (the device sorts up to %d)" % (k, MAX_MEMBERS)
    return None


def CRPS_accum(CRPS, X_f, X_o):  # noqa: N803 (the reference's parameter names)
    """Add the CRPS of the ensemble ``X_f`` ``(k, m, n, ...)`` against ``X_o`` ``(m, n, ...)`` (NumPy or DeviceArray),
    over the pixels where all members and the observation are finite, to the object ``CRPS`` made by :func:`CRPS_init`
    (or by the reference's)."""
    resident = isinstance(X_f, DeviceArray) or isinstance(X_o, DeviceArray)
    shape_f, shape_o = tuple(X_f.shape), tuple(X_o.shape)
    if len(shape_f) < 1 or shape_f[0] < 1:
        raise ValueError("need at least one array to concatenate")  # what the reference's vstack says
    k, npix = shape_f[0], _size(shape_f[1:])
    if npix != _size(shape_o):
        raise ValueError("operands could not be broadcast together with shapes (%d,) (%d,) " % (npix, _size(shape_o)))
    why = _crps_declined(k, (_dtype_of(X_f), _dtype_of(X_o)))
    if why is not None:
        return decline("CRPS_accum", why, _stock("CRPS_accum"), resident)(CRPS, X_f, X_o)
    if npix == 0:
        counts, sums = np.zeros(1, np.uint64), np.zeros((1, 2))
    else:
        counts, sums = _crps_sums(_upload(X_f), _upload(X_o), 1, k, npix, True)
    CRPS["CRPS_sum"] += np.float64(sums[0, 0] + sums[0, 1])
    CRPS["n"] += int(counts[0])


def CRPS_compute(CRPS):  # noqa: N803
    """The average of a CRPS object (NaN, with NumPy's warning, when nothing was accumulated)."""
    return 1.0 * CRPS["CRPS_sum"] / CRPS["n"]


def crps_table(X_f, X_o, return_object=False):
    """The CRPS of an ensemble against several observations in one call: ``X_f`` ``(k, m, n)`` against ``X_o`` ``(T, m,
    n)`` - or against one plane ``(m, n)`` - or ``T`` ensembles ``(T, k, m, n)`` against ``X_o`` ``(T, m, n)``.  Returns
    float64 ``(T,)`` (0-d for one plane), entry ``t`` equal to ``CRPS(X_f, X_o[t])`` (``CRPS(X_f[t], X_o[t])``) bit for
    bit; ``return_object=True`` returns ``(crps, {"CRPS_sum": (T,), "n": (T,)})``.  NumPy or DeviceArray, float32 or
    float64, at most 64 members."""
    shape_f, shape_o = tuple(X_f.shape), tuple(X_o.shape)
    single = len(shape_o) == 2
    if single:
        shape_o = (1,) + shape_o
    stacks = len(shape_f) == 4
    if len(shape_o) != 3 or len(shape_f) not in (3, 4) or shape_f[-2:] != shape_o[1:] or (stacks and shape_f[0] != shape_o[0]):
        raise ValueError("X_f must have shape (k, m, n) or (T, k, m, n) and X_o shape (m, n) or (T, m, n)")
    k, npix, planes = shape_f[-3], shape_o[1] * shape_o[2], shape_o[0]
    why = _crps_declined(k, (_dtype_of(X_f), _dtype_of(X_o)))
    if why is not None:
        raise NotImplementedError("pysteps_amd crps_table: %s is not implemented on the device" % why)
    if k < 1 or npix < 1 or planes < 1:
        raise ValueError("crps_table: empty fields")
    counts, sums = _crps_sums(_upload(X_f), _upload(X_o), planes, k, npix, not stacks)
    obj = {"CRPS_sum": sums[:, 0] + sums[:, 1], "n": counts.astype(np.float64)}
    if single:
        obj = {key: value.reshape(()) for key, value in obj.items()}
    result = CRPS_compute(obj)
    return (result, obj) if return_object else result


# ---- reliability diagram and ROC curve ------------------------------------------------------------------------------
def reldiag(P_f, X_o, X_min, n_bins=10, min_count=10):  # noqa: N803
    """The x- and y-coordinates of the points of the reliability diagram of the probabilities ``P_f`` of exceeding
    ``X_min`` against the observed values ``X_o`` (NumPy or DeviceArray of one shape)."""
    rdiag = reldiag_init(X_min, n_bins, min_count)
    reldiag_accum(rdiag, P_f, X_o)
    return reldiag_compute(rdiag)


def reldiag_init(X_min, n_bins=10, min_count=10):  # noqa: N803
    """Initialize a reliability diagram object: the reference's dict."""
    return {"X_min": X_min, "bin_edges": np.linspace(-1e-6, 1 + 1e-6, int(n_bins + 1)), "n_bins": n_bins,
            "X_sum": np.zeros(n_bins), "Y_sum": np.zeros(n_bins, dtype=int), "num_idx": np.zeros(n_bins, dtype=int),
            "sample_size": np.zeros(n_bins, dtype=int), "min_count": min_count}


def _pair(name, P_f, X_o):  # noqa: N803
    """``(npix, dtype of P_f, dtype of X_o, reason to decline or None)`` of a probability field and its observation."""
    shape_p, shape_o = tuple(P_f.shape), tuple(X_o.shape)
    if shape_p != shape_o:
        raise ValueError("%s: P_f and X_o must have one shape, got %s and %s" % (name, shape_p, shape_o))
    dt_p, dt_o = _dtype_of(P_f), _dtype_of(X_o)
    for dtype in (dt_p, dt_o):
        if dtype not in _NATIVE:
            return 0, dt_p, dt_o, "dtype %s" % dtype
    return _size(shape_p), dt_p, dt_o, None


def _edges_of(reldiag):
    """``(float64 edges, reason to decline or None)``; numpy.digitize's own error for edges in no order."""
    edges = np.ascontiguousarray(reldiag["bin_edges"], dtype=np.float64)
    np.digitize(np.empty(0), edges, right=True)
    if edges.ndim != 1 or edges.size < 2:
        return edges, "%d bin edges" % edges.size
    if edges.size - 1 > MAX_BINS:
        return edges, "%d bins (one pass counts up to %d)" % (edges.size - 1, MAX_BINS)
    if not np.all(edges[1:] >= edges[:-1]):
        return edges, "bin edges that do not increase"
    return edges, None


def _thresholds_of(ROC, dt_p):  # noqa: N803
    """``(float64 numbers the probabilities are compared with, reason to decline or None)``."""
    thrs = [_compared_as(p, dt_p) for p in ROC["prob_thrs"]]
    if len(thrs) > MAX_BINS:
        return None, "%d probability thresholds (one pass counts up to %d)" % (len(thrs), MAX_BINS)
    return np.ascontiguousarray(thrs, dtype=np.float64), None


def _add_bins(reldiag, bins, sums):
    """The reference's update: a bin with fewer than ``min_count`` pixels in this call adds zeros."""
    count = bins[:, 0].astype(int)
    keep = count >= reldiag["min_count"]
    reldiag["X_sum"] += np.where(keep, sums[:, 0] + sums[:, 1], 0.0)
    reldiag["Y_sum"] += np.where(keep, bins[:, 1].astype(int), 0)
    reldiag["num_idx"] += np.where(keep, count, 0)
    reldiag["sample_size"] += np.where(keep, count, 0)


def _add_roc(ROC, roc):  # noqa: N803
    for i in range(roc.shape[0]):
        for c, key in enumerate(("hits", "misses", "false_alarms", "corr_neg")):
            ROC[key][i] += int(roc[i, c])


def reldiag_accum(reldiag, P_f, X_o):  # noqa: N803
    """Accumulate the probability-observation pairs ``P_f``, ``X_o`` (NumPy or DeviceArray of one shape) into the
    reliability diagram object ``reldiag`` made by :func:`reldiag_init` (or by the reference's)."""
    resident = isinstance(P_f, DeviceArray) or isinstance(X_o, DeviceArray)
    npix, _, dt_o, why = _pair("reldiag_accum", P_f, X_o)
    edges = None
    if why is None:
        edges, why = _edges_of(reldiag)
    if why is not None:
        return decline("reldiag_accum", why, _stock("reldiag_accum"), resident)(reldiag, P_f, X_o)
    if npix == 0:
        bins, sums = np.zeros((edges.size - 1, 2), np.uint64), np.zeros((edges.size - 1, 2))
    else:
        bins, sums, _ = _bins(_upload(P_f), _upload(X_o), npix, _compared_as(reldiag["X_min"], dt_o), edges, None)
    _add_bins(reldiag, bins, sums)


def reldiag_compute(reldiag):
    """The x- and y-coordinates ``(r, f)`` of the points of the reliability diagram (NaN, with NumPy's warning, for a
    bin without samples)."""
    f = 1.0 * reldiag["Y_sum"] / reldiag["num_idx"]
    r = 1.0 * reldiag["X_sum"] / reldiag["num_idx"]
    return r, f


def ROC_curve(P_f, X_o, X_min, n_prob_thrs=10, compute_area=False):  # noqa: N802, N803
    """The ROC curve ``(POFD, POD)`` - and its area with ``compute_area`` - of the probabilities ``P_f`` of exceeding
    ``X_min`` against the observed values ``X_o`` (NumPy or DeviceArray of one shape)."""
    roc = ROC_curve_init(X_min, n_prob_thrs)
    ROC_curve_accum(roc, P_f, X_o)
    return ROC_curve_compute(roc, compute_area)


def ROC_curve_init(X_min, n_prob_thrs=10):  # noqa: N802, N803
    """Initialize a ROC curve object: the reference's dict."""
    return {"X_min": X_min, "hits": np.zeros(n_prob_thrs, dtype=int), "misses": np.zeros(n_prob_thrs, dtype=int),
            "false_alarms": np.zeros(n_prob_thrs, dtype=int), "corr_neg": np.zeros(n_prob_thrs, dtype=int),
            "prob_thrs": np.linspace(0.0, 1.0, int(n_prob_thrs))}


def ROC_curve_accum(ROC, P_f, X_o):  # noqa: N802, N803
    """Accumulate the probability-observation pairs ``P_f``, ``X_o`` (NumPy or DeviceArray of one shape) into the ROC
    curve object ``ROC`` made by :func:`ROC_curve_init` (or by the reference's)."""
    resident = isinstance(P_f, DeviceArray) or isinstance(X_o, DeviceArray)
    npix, dt_p, dt_o, why = _pair("ROC_curve_accum", P_f, X_o)
    thrs = None
    if why is None:
        thrs, why = _thresholds_of(ROC, dt_p)
    if why is not None:
        return decline("ROC_curve_accum", why, _stock("ROC_curve_accum"), resident)(ROC, P_f, X_o)
    if npix == 0 or thrs.size == 0:
        return None
    _, _, roc = _bins(_upload(P_f), _upload(X_o), npix, _compared_as(ROC["X_min"], dt_o), None, thrs)
    _add_roc(ROC, roc)


def _accum_both(reldiag, ROC, P_f, X_o):  # noqa: N803
    """:func:`reldiag_accum` and :func:`ROC_curve_accum` of two objects with one ``X_min`` from ONE read of the planes;
    objects the device declines raise."""
    npix, dt_p, dt_o, why = _pair("ProbScoresAccumulator", P_f, X_o)
    edges = thrs = None
    if why is None:
        edges, why = _edges_of(reldiag)
    if why is None:
        thrs, why = _thresholds_of(ROC, dt_p)
    if why is not None or npix == 0 or thrs.size == 0 or reldiag["X_min"] != ROC["X_min"]:
        raise NotImplementedError("pysteps_amd ProbScoresAccumulator: %s is not implemented on the device"
                                  % (why or "an empty field, no probability threshold or two intensity thresholds"))
    bins, sums, roc = _bins(_upload(P_f), _upload(X_o), npix, _compared_as(ROC["X_min"], dt_o), edges, thrs)
    _add_bins(reldiag, bins, sums)
    _add_roc(ROC, roc)


def ROC_curve_compute(ROC, compute_area=False):  # noqa: N802, N803
    """The ROC curve of a ROC curve object: the lists ``(POFD, POD)`` over its probability thresholds and, with
    ``compute_area``, the area under the curve as the third element."""
    n = len(ROC["prob_thrs"])
    POD_vals = [1.0 * ROC["hits"][i] / (ROC["hits"][i] + ROC["misses"][i]) for i in range(n)]  # noqa: N806
    POFD_vals = [1.0 * ROC["false_alarms"][i] / (ROC["corr_neg"][i] + ROC["false_alarms"][i]) for i in range(n)]  # noqa: N806
    if not compute_area:
        return POFD_vals, POD_vals
    # the parallelepipeds under the curve, from (1, 1) down to (0, 0)
    area = (1.0 - POFD_vals[0]) * (1.0 + POD_vals[0]) / 2.0
    for i in range(n - 1):
        area += (POFD_vals[i] - POFD_vals[i + 1]) * (POD_vals[i + 1] + POD_vals[i]) / 2.0
    area += POFD_vals[-1] * POD_vals[-1] / 2.0
    return POFD_vals, POD_vals, area


class ProbScoresAccumulator:
    """Probabilistic scores of an ensemble nowcast against the observations of its lead times, usable as the
    ``callback`` of a nowcast::

        acc = ProbScoresAccumulator(observations, [0.1, 1.0, 5.0])
        nowcasts.get_method("steps")(..., callback=acc, return_output=False)
        acc.crps()               # (n_leadtimes,)
        acc.reldiag(t, i)        # (r, f) of lead time t and intensity threshold i
        acc.roc(t, i, True)      # (POFD, POD, area)
        acc.crps_objects[t], acc.reldiag_objects[t][i], acc.roc_objects[t][i]

    ``observations`` is ``(n_leadtimes, m, n)``, NumPy or DeviceArray, and is kept on the device.  Call ``t`` receives
    the members of lead time ``t`` - a ``DeviceArray`` ``(k, m, n)`` from the resident nowcast loop, a host ``ndarray``
    from any other - and adds them to one CRPS object (``crps=False``: none) and, for every intensity threshold of
    ``thrs``, to one reliability diagram (``n_bins``, ``min_count``) and one ROC curve (``n_prob_thrs``) whose ``X_min``
    is that threshold.  The probabilities are the planes of
    :func:`pysteps_amd.postprocessing.ensemblestats.excprob` of the members (``ignore_nan`` is its option): they are made
    on the device and stay there, so the objects equal those of ``excprob`` followed by the ``_accum`` functions, and
    with ``return_output=False`` neither a member nor a probability plane leaves HBM."""

    accepts_device = True

    def __init__(self, observations, thrs, n_bins=10, n_prob_thrs=10, min_count=10, crps=True, ignore_nan=False):
        self.thrs = [thrs] if np.isscalar(thrs) else list(thrs)
        if not self.thrs and not crps:
            raise ValueError("ProbScoresAccumulator: no threshold and no CRPS requested")
        if len(observations.shape) != 3:
            raise ValueError("ProbScoresAccumulator: observations of shape (n_leadtimes, m, n) expected, got %s"
                             % (tuple(observations.shape),))
        self._obs = observations if isinstance(observations, DeviceArray) else DeviceArray.from_host(np.asarray(observations))
        self.n_bins, self.n_prob_thrs, self.min_count = n_bins, n_prob_thrs, min_count
        self.with_crps, self.ignore_nan = bool(crps), ignore_nan
        self.crps_objects = []
        self.reldiag_objects = []
        self.roc_objects = []
        self.n_leadtimes = 0
        self.received = []  # type of the members of every call: DeviceArray or ndarray

    def __call__(self, members):
        from ..postprocessing import ensemblestats  # noqa: PLC0415

        resident = isinstance(members, DeviceArray)
        self.received.append(DeviceArray if resident else np.ndarray)
        if not resident:
            members = np.asarray(members)
        if len(members.shape) != 3 or tuple(members.shape[1:]) != self._obs.shape[1:]:
            raise ValueError("ProbScoresAccumulator: members of shape (k, %d, %d) expected, got %s"
                             % (self._obs.shape[1:] + (tuple(members.shape),)))
        if self.n_leadtimes >= self._obs.shape[0]:
            raise ValueError("ProbScoresAccumulator: called for more lead times than the %d observations" % self._obs.shape[0])
        obs = self._obs.view(self.n_leadtimes)
        dev = _upload(members)  # one upload serves both kernels
        if self.with_crps:
            crps = CRPS_init()
            CRPS_accum(crps, dev, obs)
            self.crps_objects.append(crps)
        diagrams, curves = [], []
        if self.thrs:
            probs = ensemblestats.excprob(dev, self.thrs, ignore_nan=self.ignore_nan)  # (nthr, m, n) float64, resident
            for i, thr in enumerate(self.thrs):
                diagrams.append(reldiag_init(thr, self.n_bins, self.min_count))
                curves.append(ROC_curve_init(thr, self.n_prob_thrs))
                _accum_both(diagrams[i], curves[i], probs.view(i), obs)
        self.reldiag_objects.append(diagrams)
        self.roc_objects.append(curves)
        self.n_leadtimes += 1

    def crps(self):
        """The CRPS of every lead time: float64 ``(n_leadtimes,)`` (NaN where no pixel took part)."""
        with np.errstate(all="ignore"):
            return np.array([CRPS_compute(obj) for obj in self.crps_objects], dtype=np.float64)

    def reldiag(self, t, i):
        """``(r, f)`` of the reliability diagram of lead time ``t`` and intensity threshold ``i``."""
        with np.errstate(all="ignore"):
            return reldiag_compute(self.reldiag_objects[t][i])

    def roc(self, t, i, compute_area=False):
        """``(POFD, POD[, area])`` of the ROC curve of lead time ``t`` and intensity threshold ``i``."""
        with np.errstate(all="ignore"):
            return ROC_curve_compute(self.roc_objects[t][i], compute_area)
