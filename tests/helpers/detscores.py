"""Independent restatement of what pysteps/verification/detcatscores.py ``det_cat_fct_accum`` counts and
pysteps/verification/detcontscores.py ``det_cont_fct_accum`` averages (test yardstick), and the generators of the test
fields.

Counts are Python integers.  The raw sums are ``math.fsum`` over float64 terms formed from the widened inputs (one
rounding per term: the residual, the pair sum, their squares, the product), returned with the sum of the terms'
magnitudes, which scales the bar of a comparison.  The nine quantities of the verification error object are evaluated
from their definitions in ``numpy.longdouble``.
"""

import math

import numpy as np

THRESHOLDS = [0.5, 1.0, 1.0e6, -1.0]  # Python floats; no pixel exceeds 1e6, every pixel of a field without NaN exceeds -1
CONT_THR = 0.5
CONDITIONINGS = [None, "single", "double"]
MOMENTS = ["cov", "vobs", "vpred", "mobs", "mpred", "me", "mse", "mss", "mae"]  # the object's arrays; "n" follows
CAT_KEYS = ["hits", "misses", "false_alarms", "correct_negatives"]
CAT_SCORES = ["POD", "FAR", "FA", "ACC", "CSI", "BIAS", "HSS", "HK", "GSS", "SEDI", "MCC", "F1"]
CONT_SCORES = ["ME", "MAE", "MSE", "NMSE", "RMSE", "corr_p", "beta1", "beta2", "DRMSE", "RV"]
SUMS = ["res", "res2", "abs", "sum2", "obs_pair", "pred_pair", "obs_pred", "obs", "obs2", "pred", "pred2"]  # the kernel's order


def field(m, n, seed, dtype=np.float32, wet=0.45, nan=0.0):
    """A rain-like field: gamma-distributed intensities over a dry background, every value a float32 number; a fraction
    ``nan`` of the pixels is NaN."""
    rng = np.random.default_rng(seed)
    x = np.where(rng.random((m, n)) < wet, rng.gamma(0.8, 3.0, (m, n)), 0.0).astype(np.float32)
    if nan:
        x[rng.random((m, n)) < nan] = np.nan
    return x.astype(dtype)


def pair(m, n, seed, dtype=np.float32, nan_f=0.0, nan_o=0.0):
    """(forecast, observation): the observation is the forecast's clean twin displaced and perturbed."""
    f = field(m, n, seed, np.float32, nan=nan_f)
    rng = np.random.default_rng(seed + 5000)
    base = np.roll(field(m, n, seed, np.float32), (1, -2), axis=(0, 1))
    o = (base * rng.uniform(0.5, 1.5, (m, n)) + np.where(rng.random((m, n)) < 0.05, rng.gamma(0.8, 3.0, (m, n)), 0.0)).astype(np.float32)
    if nan_o:
        o[rng.random((m, n)) < nan_o] = np.nan
    return f.astype(dtype), o.astype(dtype)


def counts(pred, obs, thr):
    """(hits, misses, false alarms, correct negatives) as Python integers; ``> thr`` as NumPy compares an array of the
    field's dtype with ``thr``, NaN comparing false."""
    pred, obs = np.asarray(pred), np.asarray(obs)
    with np.errstate(invalid="ignore"):
        pb, ob = (pred > thr).ravel().tolist(), (obs > thr).ravel().tolist()
    h = sum(1 for p, o in zip(pb, ob) if p and o)
    m = sum(1 for p, o in zip(pb, ob) if not p and o)
    f = sum(1 for p, o in zip(pb, ob) if p and not o)
    return h, m, f, len(pb) - h - m - f


def conditioned(pred, obs, conditioning=None, thr=0.0):
    """float64 copies of both fields with the pixels the conditioning excludes set to NaN on both sides; the comparison
    is made in each field's own dtype."""
    pred, obs = np.asarray(pred), np.asarray(obs)
    p, o = pred.astype(np.float64), obs.astype(np.float64)
    if conditioning is not None:
        with np.errstate(invalid="ignore"):
            pb, ob = pred > thr, obs > thr
        keep = (pb | ob) if conditioning == "single" else (pb & ob)
        p[~keep] = np.nan
        o[~keep] = np.nan
    return p.ravel(), o.ravel()


def raw_sums(pred, obs, conditioning=None, thr=0.0):
    """``(counts, sums, magnitudes)``: the numbers of finite observations, finite predictions and finite pairs; per
    name of ``SUMS`` the ``math.fsum`` of the float64 terms, and the sum of their absolute values (longdouble: it only
    scales a bar)."""
    p, o = conditioned(pred, obs, conditioning, thr)
    fo, fp = np.isfinite(o), np.isfinite(p)
    both = fo & fp
    pp, oo = p[both], o[both]
    res, tot = pp - oo, pp + oo
    terms = {"res": res, "res2": res * res, "abs": np.abs(res), "sum2": tot * tot, "obs_pair": oo, "pred_pair": pp,
             "obs_pred": oo * pp, "obs": o[fo], "obs2": o[fo] * o[fo], "pred": p[fp], "pred2": p[fp] * p[fp]}
    sums = {k: math.fsum(v.tolist()) for k, v in terms.items()}
    mags = {k: float(np.sum(np.abs(v), dtype=np.longdouble)) for k, v in terms.items()}
    return (int(fo.sum()), int(fp.sum()), int(both.sum())), sums, mags


def moments(pred, obs, conditioning=None, thr=0.0):
    """The nine quantities of the error object and ``n`` from their definitions, in numpy.longdouble: means of the
    residual, its square, the squared pair sum and the absolute residual over the pairs; the mean of each field over
    its own finite pixels, the mean squared deviation from it over the same pixels, and the mean product of the
    deviations over the pairs."""
    p, o = conditioned(pred, obs, conditioning, thr)
    p, o = p.astype(np.longdouble), o.astype(np.longdouble)
    fo, fp = np.isfinite(o), np.isfinite(p)
    both = fo & fp
    n = int(both.sum())
    res, tot = p[both] - o[both], p[both] + o[both]
    mobs, mpred = o[fo].sum() / fo.sum(), p[fp].sum() / fp.sum()
    out = {"mobs": mobs, "mpred": mpred, "vobs": ((o[fo] - mobs) ** 2).sum() / fo.sum(),
           "vpred": ((p[fp] - mpred) ** 2).sum() / fp.sum(), "cov": ((o[both] - mobs) * (p[both] - mpred)).sum() / n,
           "me": res.sum() / n, "mse": (res * res).sum() / n, "mss": (tot * tot).sum() / n, "mae": np.abs(res).sum() / n}
    return out, n


def reference_deviation(obj, pred, obs, conditioning, thr=CONT_THR):
    """The largest relative deviation of the moments of a single-accumulation error object ``obj`` - (10,) or (10, K):
    ``MOMENTS`` then ``n`` - from their longdouble definitions; a quantity whose definition gives exactly zero has to be
    zero."""
    obj, pred, obs = np.asarray(obj), np.asarray(pred), np.asarray(obs)
    if obj.ndim == 2:
        return max(reference_deviation(obj[:, k], pred[k], obs[k], conditioning, thr) for k in range(obj.shape[1]))
    want, n = moments(pred, obs, conditioning, thr)
    assert int(obj[len(MOMENTS)]) == n
    worst = 0.0
    for i, key in enumerate(MOMENTS):
        if want[key] == 0:
            assert obj[i] == 0.0, key
        else:
            worst = max(worst, float(abs((np.longdouble(obj[i]) - want[key]) / want[key])))
    return worst
