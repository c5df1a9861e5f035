"""Independent restatement of pysteps/verification/ensscores.py ``ensemble_skill`` and ``ensemble_spread`` (test
yardstick), and the generators of the test stacks.

Pairs come in the reference's loop order - member i outer, member j > i inner; member i is the prediction, member j the
observation.  Contingency tables of the pairs are Python integers, counted directly or through the ballot identity the
kernel uses: with the event bits of a member packed into words, hits(i, j) is the population count of ``b_i & b_j`` and
the other three entries follow from it, the two members' numbers of events and the number of pixels.  Categorical scores
are the reference's float64 formulas on those integers.  Continuous scores are evaluated from ``math.fsum`` sums
(tests/helpers/detscores.py) in exact rational arithmetic up to the final formula, the FSS from the integer sums of
tests/helpers/fss.py as an exact rational rounded once.
"""

from fractions import Fraction

import numpy as np

from . import detscores as det
from . import fss as fss_helper

CAT_METRICS = ["CSI", "POD", "FAR", "BIAS"]
CAT_THRESHOLDS = [0.5, 2.0]  # Python floats
CONT_METRICS = ["RMSE", "MAE", "ME", "corr_p", "NMSE", "DRMSE", "RV", "beta1"]
FSS_KWARGS = {"thr": 0.5, "scale": 3}
CONDITIONED = [("RMSE", {"conditioning": "single", "thr": 0.5}), ("corr_p", {"conditioning": "double", "thr": 0.5})]
NAN_PATTERNS = ["none", "border", "allnan", "onepixel"]
# (name, K, shape, NaN pattern): every K, shape and pattern of the list at least once
CASES = [("k2_1x1_none", 2, (1, 1), "none"), ("k3_7x9_border", 3, (7, 9), "border"), ("k9_7x9_none", 9, (7, 9), "none"),
         ("k5_7x9_onepixel", 5, (7, 9), "onepixel"), ("k5_33x47_none", 5, (33, 47), "none"),
         ("k9_33x47_border", 9, (33, 47), "border"), ("k3_33x47_allnan", 3, (33, 47), "allnan"),
         ("k2_64x65_border", 2, (64, 65), "border"), ("k3_64x65_none", 3, (64, 65), "none"),
         ("k5_64x65_onepixel", 5, (64, 65), "onepixel")]
CONDITIONED_CASE = "k5_33x47_none"


def metrics():
    """``[(label, metric, kwargs)]`` of the golden file, in its order."""
    out = [("%s_%g" % (m, thr), m, {"thr": thr}) for m in CAT_METRICS for thr in CAT_THRESHOLDS]
    out += [(m, m, {}) for m in CONT_METRICS]
    out.append(("fss", "fss", dict(FSS_KWARGS)))
    return out


def pair_order(K):
    """The pairs (i, j) in the reference's loop order."""
    return [(i, j) for i in range(K) for j in range(i + 1, K)]


def members(K, m, n, seed, dtype=np.float32, pattern="none"):
    """``(stack (K, m, n), observation (m, n))``: members are one rain-like field perturbed, every value a float32
    number.  ``border``: member k is NaN in a frame of its own width (k % 3 + 1 pixels, clipped to the field);
    ``allnan``: member 1 is NaN everywhere; ``onepixel``: at one pixel every member but one is NaN."""
    rng = np.random.default_rng(seed)
    base = det.field(m, n, seed, np.float32)
    stack = np.empty((K, m, n), dtype=np.float32)
    for k in range(K):
        noise = np.where(rng.random((m, n)) < 0.05, rng.gamma(0.8, 3.0, (m, n)), 0.0)
        stack[k] = (np.roll(base, (k % 2, -(k % 3)), axis=(0, 1)) * rng.uniform(0.5, 1.5, (m, n)) + noise).astype(np.float32)
    obs = (np.roll(base, (1, 1), axis=(0, 1)) * rng.uniform(0.7, 1.3, (m, n))).astype(np.float32)
    if pattern == "border":
        for k in range(K):
            w = k % 3 + 1
            frame = np.ones((m, n), dtype=bool)
            frame[w:m - w, w:n - w] = False
            stack[k][frame] = np.nan
    elif pattern == "allnan":
        stack[1] = np.nan
    elif pattern == "onepixel":
        stack[:, m // 2, n // 3] = np.nan
        stack[K - 1, m // 2, n // 3] = np.float32(1.5)
    elif pattern != "none":
        raise ValueError(pattern)
    return stack.astype(dtype), obs.astype(dtype)


def events(stack, thr):
    """bool ``(K, npix)``: ``> thr`` as NumPy compares an array of the stack's dtype with ``thr``, NaN false."""
    stack = np.asarray(stack)
    with np.errstate(invalid="ignore"):
        return (stack > thr).reshape(stack.shape[0], -1)


_POPCOUNT = np.array([bin(b).count("1") for b in range(256)], dtype=np.int64)


def ballot_tables(stack, thr):
    """The contingency tables (hits, misses, false alarms, correct negatives) of every pair as Python integers, from
    packed event bits: hits = popcount(b_i & b_j), false alarms = n_i - hits, misses = n_j - hits, correct negatives =
    npix - n_i - n_j + hits."""
    bits = events(stack, thr)
    npix = bits.shape[1]
    words = np.packbits(bits, axis=1)
    n = [int(_POPCOUNT[w].sum()) for w in words]
    out = []
    for i, j in pair_order(bits.shape[0]):
        hits = int(_POPCOUNT[words[i] & words[j]].sum())
        out.append((hits, n[j] - hits, n[i] - hits, npix - n[i] - n[j] + hits))
    return out


def direct_tables(stack, thr):
    """The same tables counted pixel by pixel (tests/helpers/detscores.py ``counts``), member i against member j."""
    stack = np.asarray(stack)
    return [det.counts(stack[i], stack[j], thr) for i, j in pair_order(stack.shape[0])]


def cat_score(table, metric):
    """The reference's formula on (hits, misses, false alarms, correct negatives), in float64."""
    H, M, F, _ = (np.float64(1.0 * c) for c in table)
    with np.errstate(all="ignore"):
        return {"CSI": lambda: H / (H + M + F), "POD": lambda: H / (H + M), "FAR": lambda: F / (H + F),
                "BIAS": lambda: (H + F) / (H + M)}[metric]()


def pair_moments(pred, obs, conditioning=None, thr=0.0):
    """``(moments, n)`` of the error object after one accumulation of (pred, obs): exact rationals of the ``math.fsum``
    sums (means over the pairs with a finite residual; each field's mean and mean squared deviation over its own finite
    pixels; the mean product of the deviations over the pairs).  The reference merges a batch with its pair count as
    the weight, so a batch without a pair leaves the zeros of a fresh object."""
    (n_obs, n_pred, n), S, _ = det.raw_sums(pred, obs, conditioning, thr)
    if n == 0:
        return dict.fromkeys(det.MOMENTS, Fraction(0)), 0
    S = {k: Fraction(v) for k, v in S.items()}
    mobs, mpred = S["obs"] / n_obs, S["pred"] / n_pred
    out = {"mobs": mobs, "mpred": mpred, "vobs": S["obs2"] / n_obs - mobs * mobs, "vpred": S["pred2"] / n_pred - mpred * mpred,
           "cov": (S["obs_pred"] - mobs * S["pred_pair"] - mpred * S["obs_pair"]) / n + mobs * mpred,
           "me": S["res"] / n, "mse": S["res2"] / n, "mss": S["sum2"] / n, "mae": S["abs"] / n}
    return out, n


def cont_score(pred, obs, metric, conditioning=None, thr=0.0):
    """A continuous score from :func:`pair_moments`: rational up to the square roots, which are taken of the correctly
    rounded float64 radicand."""
    mo, _ = pair_moments(pred, obs, conditioning, thr)
    f = lambda x: np.float64(float(x))  # noqa: E731
    with np.errstate(all="ignore"):
        if metric == "ME":
            return f(mo["me"])
        if metric == "MAE":
            return f(mo["mae"])
        if metric == "RMSE":
            return np.sqrt(f(mo["mse"]))
        if metric == "NMSE":
            return f(mo["mse"] / mo["mss"]) if mo["mss"] else f(mo["mse"]) / f(mo["mss"])
        if metric == "DRMSE":
            return np.sqrt(f(mo["mse"] - mo["me"] ** 2))
        if metric == "RV":
            return f(1 - mo["mse"] / mo["vobs"]) if mo["vobs"] else np.float64(1.0) - f(mo["mse"]) / f(mo["vobs"])
        if metric == "beta1":
            return f(mo["cov"] / mo["vpred"]) if mo["vpred"] else f(mo["cov"]) / f(mo["vpred"])
        if metric == "corr_p":
            return f(mo["cov"]) / np.sqrt(f(mo["vobs"])) / np.sqrt(f(mo["vpred"]))
    raise ValueError(metric)


def fss_score(pred, obs, thr, scale):
    """The FSS as an exact rational of the integer window sums, rounded once (NaN for an all-dry pair)."""
    ff, fo, oo = fss_helper.sums(pred, obs, thr, scale)
    if ff + oo == 0:
        return np.float64(np.nan)
    return np.float64(float(1 - Fraction(ff - 2 * fo + oo, ff + oo)))


def score(pred, obs, metric, **kwargs):
    """One deterministic score of (pred, obs) by this module's restatement."""
    if metric in CAT_METRICS:
        return cat_score(det.counts(pred, obs, kwargs["thr"]), metric)
    if metric == "fss":
        return fss_score(pred, obs, kwargs["thr"], kwargs["scale"])
    return cont_score(pred, obs, metric, kwargs.get("conditioning"), kwargs.get("thr", 0.0))


def pair_scores(stack, metric, **kwargs):
    """float64 ``(K, K)``: entry [i, j], i < j, the score of member i against member j; NaN elsewhere."""
    stack = np.asarray(stack)
    K = stack.shape[0]
    out = np.full((K, K), np.nan, dtype=np.float64)
    for i, j in pair_order(K):
        out[i, j] = score(stack[i], stack[j], metric, **kwargs)
    return out


def ensemble_spread(stack, metric, **kwargs):
    stack = np.asarray(stack)
    with np.errstate(all="ignore"):
        return np.mean([score(stack[i], stack[j], metric, **kwargs) for i, j in pair_order(stack.shape[0])])


def ensemble_skill(stack, obs, metric, **kwargs):
    stack = np.asarray(stack)
    with np.errstate(all="ignore"):
        return np.mean([score(stack[k], obs, metric, **kwargs) for k in range(stack.shape[0])])


def lost(reference, exact):
    """Where the reference returns NaN for a score whose restatement is finite: its own rounding took the value (the
    square root of a difference that cancels to a negative residue, as DRMSE of a single pixel in float32)."""
    reference, exact = np.asarray(reference, dtype=np.float64), np.asarray(exact, dtype=np.float64)
    return np.isnan(reference) & np.isfinite(exact)


def deviation(got, want, skip=None):
    """The largest relative deviation of ``got`` from ``want`` where both are finite and ``want`` is not zero; NaN and
    infinite positions have to agree, and where ``want`` is zero ``got`` has to be.  Positions of ``skip`` are left
    out."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if skip is not None:
        got, want = got[~skip], want[~skip]
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
    g, w = got[fin], want[fin]
    assert np.all(g[w == 0] == 0.0)
    return float(np.max(np.abs(g[w != 0] - w[w != 0]) / np.abs(w[w != 0]), initial=0.0))


def held(got, reference, exact, bar):
    """``got`` against the reference's result within ``bar`` relative, NaN and infinite positions equal; where the
    reference lost a value (:func:`lost`) ``got`` is held to the restatement instead.  Returns the worst deviation."""
    got = np.asarray(got, dtype=np.float64)
    gone = lost(reference, exact)
    worst = max(deviation(got, reference, skip=gone), deviation(got[gone], np.asarray(exact, dtype=np.float64)[gone]))
    assert worst <= bar, (worst, bar)
    return worst
