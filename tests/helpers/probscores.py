"""Independent restatement of what pysteps/verification/probscores.py ``CRPS_accum``, ``reldiag_accum`` and
``ROC_curve_accum`` add to their objects (test yardstick), and the generators of the test fields.

CRPS: per pixel whose members and observation are all finite, the members are sorted and the K + 1 bins walked with
strict inequalities; a bin gives the terms ``alpha * w_a`` and ``beta * w_b`` with ``w_a = (i/K)**2`` and ``w_b =
((K-i)/K)**2`` (one division, one product), the differences float64 operations on the widened values.  The terms of
all pixels are added by ``math.fsum`` and returned with the sum of their magnitudes, which scales the bar of a
comparison.  :func:`crps_exact` evaluates the same rule in ``numpy.longdouble``.  The binning is plain integer counting
over a Python loop: bin ``k`` holds ``edges[k-1] < p <= edges[k]`` (the number of edges below ``p``, by bisection).
"""

import bisect
import math

import numpy as np

LEVELS = (0.0, 0.5, 1.0, 2.0)
MEMBER_COUNTS = (1, 2, 3, 7, 20, 48, 64)
ROC_KEYS = ("hits", "misses", "false_alarms", "corr_neg")
BIN_KEYS = ("X_sum", "Y_sum", "num_idx", "sample_size")


def quantised(shape, seed, dtype=np.float32):
    """A field of four levels with about 60 % zeros: almost every comparison between two of them is a tie."""
    rng = np.random.default_rng(seed)
    return rng.choice(LEVELS, size=shape, p=(0.6, 0.15, 0.15, 0.1)).astype(dtype)


def rainy(shape, seed, dtype=np.float32):
    """Gamma-distributed intensities over a dry background, every value a float32 number."""
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < 0.45, rng.gamma(0.8, 3.0, shape), 0.0).astype(np.float32).astype(dtype)


def ensemble(K, m, n, seed, dtype=np.float32, ties=True, bad=False):
    """``(members (K, m, n), observation (m, n))``.  ``bad`` puts NaN, +inf and -inf into member ``K // 2`` at pixels
    0, 1, 2 and into the observation at pixels 3, 4, 5 (planes of at least 7 pixels)."""
    make = quantised if ties else rainy
    members, obs = make((K, m, n), seed, dtype), make((m, n), seed + 1000, dtype)
    if bad and m * n >= 7:
        for pixel, value in enumerate((np.nan, np.inf, -np.inf)):
            members.reshape(K, -1)[K // 2, pixel] = value
            obs.reshape(-1)[3 + pixel] = value
    return members, obs


def tie_pixels(K, dtype=np.float32):
    """``(members (K, 1, 9), observation (1, 9))`` of the cases named by the issue: the observation equal to the
    smallest, the largest and a middle member (pixels 0-2), all members equal with the observation below, equal and
    above (3-5), distinct members with the observation strictly between two of them, below all and above all (6-8)."""
    rng = np.random.default_rng(K)
    distinct = rng.permutation(np.arange(1, K + 1)).astype(np.float64) * 0.25
    members = np.empty((K, 9), dtype=np.float64)
    obs = np.empty(9, dtype=np.float64)
    for pixel in (0, 1, 2, 6, 7, 8):
        members[:, pixel] = distinct
    ordered = np.sort(distinct)
    obs[0], obs[1], obs[2] = ordered[0], ordered[-1], ordered[K // 2]
    members[:, 3:6] = 1.5
    obs[3:6] = (0.75, 1.5, 3.0)
    obs[6], obs[7], obs[8] = ordered[(K - 1) // 2] + 0.125, 0.0, ordered[-1] + 1.0
    return members.astype(dtype).reshape(K, 1, 9), obs.astype(dtype).reshape(1, 9)


def crps_weights(K):
    """Python floats ``[(w_a, w_b)]`` of the K + 1 bins."""
    out = []
    for i in range(K + 1):
        p, q = float(i) / float(K), float(K - i) / float(K)
        out.append((p * p, q * q))
    return out


def _sorted_finite(members, obs, as_type):
    members, obs = np.asarray(members), np.asarray(obs)
    K = members.shape[0]
    x = members.reshape(K, -1).astype(as_type)
    o = obs.reshape(-1).astype(as_type)
    keep = np.isfinite(x).all(axis=0) & np.isfinite(o)
    return np.sort(x[:, keep], axis=0), o[keep], K


def _bin_terms(x, o, K, weights):
    """The nonzero terms of every bin: arrays in the type of ``x``."""
    zero = np.zeros_like(o)
    terms = [np.where(o < x[0], (x[0] - o) * weights[0][1], zero)]
    for i in range(1, K):
        lo, hi = x[i - 1], x[i]
        above, inside, below = o > hi, (hi > o) & (o > lo), o < lo
        alpha = np.where(above, hi - lo, np.where(inside, o - lo, zero))
        beta = np.where(below, hi - lo, np.where(inside, hi - o, zero))
        terms += [alpha * weights[i][0], beta * weights[i][1]]
    terms.append(np.where(x[K - 1] < o, (o - x[K - 1]) * weights[K][0], zero))
    return terms


def crps_terms(members, obs):
    """``(n, sum, magnitude)``: the number of pixels that take part, the ``math.fsum`` of the float64 terms and the sum
    of their absolute values."""
    x, o, K = _sorted_finite(members, obs, np.float64)
    flat = np.concatenate(_bin_terms(x, o, K, crps_weights(K))).tolist()
    return int(o.size), math.fsum(flat), math.fsum(abs(t) for t in flat)


def crps_exact(members, obs):
    """``(n, sum)`` with the sum evaluated in numpy.longdouble, the weights too."""
    x, o, K = _sorted_finite(members, obs, np.longdouble)
    k = np.longdouble(K)
    weights = [((np.longdouble(i) / k) ** 2, (np.longdouble(K - i) / k) ** 2) for i in range(K + 1)]
    total = np.longdouble(0)
    for t in _bin_terms(x, o, K, weights):
        total += t.sum(dtype=np.longdouble)
    return int(o.size), total


def bin_counts(P_f, X_o, X_min, edges=None, prob_thrs=None):
    """What one ``_accum`` call sees, before ``min_count``: per bin the number of pixels (``count``), of those with
    ``X_o >= X_min`` (``events``), the ``math.fsum`` of their probabilities (``sum``) and of the magnitudes
    (``magnitude``); per probability threshold ``[hits, misses, false alarms, correct negatives]`` (``roc``).  The
    comparisons with ``X_min`` and the thresholds are NumPy's, element by element; all counting is Python's."""
    P_f, X_o = np.asarray(P_f).reshape(-1), np.asarray(X_o).reshape(-1)
    with np.errstate(invalid="ignore"):
        valid = (np.isfinite(P_f) & np.isfinite(X_o)).tolist()
        event = (X_o >= X_min).tolist()
        ge = [(P_f >= p).tolist() for p in (prob_thrs if prob_thrs is not None else [])]
    out = {}
    if edges is not None:
        edge_list = [float(e) for e in edges]
        n_bins = len(edge_list) - 1
        count, events, members = [0] * n_bins, [0] * n_bins, [[] for _ in range(n_bins)]
        for idx, p in enumerate(P_f.tolist()):
            if not valid[idx]:
                continue
            k = bisect.bisect_left(edge_list, p)  # the number of edges below p
            if 1 <= k <= n_bins:
                count[k - 1] += 1
                events[k - 1] += 1 if event[idx] else 0
                members[k - 1].append(p)
        out.update(count=count, events=events, sum=[math.fsum(v) for v in members],
                   magnitude=[math.fsum(abs(p) for p in v) for v in members])
    if prob_thrs is not None:
        roc = []
        for row in ge:
            table = [0, 0, 0, 0]
            for idx, yes in enumerate(row):
                if valid[idx]:
                    table[(0 if yes else 1) if event[idx] else (2 if yes else 3)] += 1
            roc.append(table)
        out["roc"] = roc
    return out


def add_to_reldiag(total, counted, min_count):
    """Add one call's bins to ``total`` (dict of lists ``X_sum``, ``X_mag``, ``Y_sum``, ``num_idx``, ``sample_size``;
    created when None) as the reference does: a bin with fewer than ``min_count`` pixels in the call adds zeros.
    ``X_sum`` collects the calls' sums, added with ``math.fsum`` by :func:`reldiag_x_sum`."""
    n_bins = len(counted["count"])
    if total is None:
        total = {"X_sum": [[] for _ in range(n_bins)], "X_mag": [0.0] * n_bins, "Y_sum": [0] * n_bins, "num_idx": [0] * n_bins,
                 "sample_size": [0] * n_bins}
    for b in range(n_bins):
        if counted["count"][b] >= min_count:
            total["X_sum"][b].append(counted["sum"][b])
            total["X_mag"][b] += counted["magnitude"][b]
            total["Y_sum"][b] += counted["events"][b]
            total["num_idx"][b] += counted["count"][b]
            total["sample_size"][b] += counted["count"][b]
    return total


def reldiag_x_sum(total):
    return [math.fsum(v) for v in total["X_sum"]]


def probabilities(K, shape, seed, dtype=np.float64):
    """A plane of probabilities ``j/K``, j = 0..K, every value equally likely: 0.0, 1.0 and values on bin edges."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, K + 1, size=shape) / np.float64(K)).astype(dtype)
