"""Golden vectors for ensemble skill and spread (``pysteps_amd.verification.ensscores``), written by the UNMODIFIED
reference.

    python tools/make_golden_ensscores.py        (-> tests/golden/ensscores_reference.npz)

Runs ``ensemble_skill`` and ``ensemble_spread`` of the reference package that ``oracle.build_ref`` prepares under
oracle/_ref, and its ``get_method(metric, type="deterministic")`` on every pair of members.  Stacks are stored as float32
(every value is a float32 number, so the float64 run uses the same numbers widened).  ``cases`` names the stacks of
tests/helpers/ensscores.py ``CASES`` (K = 2, 3, 5, 9; shapes (1, 1), (7, 9), (33, 47), (64, 65); NaN patterns none, a
different NaN border per member, one member all NaN, one pixel finite in exactly one member), ``labels`` the metrics of
its ``metrics()``: CSI, POD, FAR and BIAS at two thresholds, eight continuous scores, the FSS at one threshold and
scale.  ``<...>__exact_skill / exact_spread / exact_pairs`` beside each of the three results below are the same
quantities by the restatement of tests/helpers/ensscores.py; ``reference_lost`` counts the results for which the reference
returns NaN where the restatement is finite (the square root of a difference its own rounding made negative: DRMSE of a
single pixel in float32) - they are left out of the deviations and the tests hold the device to the restatement there.
Per case ``<case>__x`` (K, m, n) and ``<case>__o`` (m, n); per case and dtype

    <case>__<dtype>__skill     (nmetric,)        ensemble_skill against <case>__o
    <case>__<dtype>__spread    (nmetric,)        ensemble_spread
    <case>__<dtype>__pairs     (nmetric, K, K)   the score of member i against member j at [i, j], i < j; NaN elsewhere
    <case>__<dtype>__tables    (nthr, pairs, 4)  hits, misses, false alarms, correct negatives of every pair

and for ``conditioned_case`` ``<case>__<dtype>__cond_<i>__skill / spread / pairs`` for the two conditioned calls of
``CONDITIONED``.  ``messages`` holds the texts of the reference's errors (2-D ``X_f``, one member, a shape mismatch, a
lower-case metric).  ``deviation_float32`` / ``deviation_float64`` are the largest relative deviations of a continuous
score of the reference - per pair, per member, spread and skill, conditioned calls included - from the restatement of
tests/helpers/ensscores.py (``math.fsum`` sums, exact rationals), per dtype of the stack; ``deviation_fss`` the same for
the FSS, both dtypes.  The GPU tests allow 5 x these.  Needs the reference; never runs on the GPU machine.
"""
import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUT = os.path.join(ROOT, "tests", "golden", "ensscores_reference.npz")


def main():
    from helpers import ensscores as restated
    from oracle import build_ref

    build_ref.build()
    build_ref.activate()
    from pysteps.verification import detcatscores as cat
    from pysteps.verification import ensscores as ens
    from pysteps.verification.interface import get_method

    metrics = restated.metrics()
    out = {"versions": np.array(json.dumps({"numpy": np.__version__})), "cases": np.array([c[0] for c in restated.CASES]),
           "labels": np.array([m[0] for m in metrics]), "cat_thresholds": np.array(restated.CAT_THRESHOLDS, dtype=np.float64),
           "conditioned_case": np.array(restated.CONDITIONED_CASE)}
    deviation = {"float32": 0.0, "float64": 0.0, "fss": 0.0}

    def reference(x, o, metric, kwargs):
        """(skill, spread, pairs) of the reference, and the same three of the restatement."""
        fn = get_method(metric, type="deterministic")
        K = x.shape[0]
        pairs = np.full((K, K), np.nan)
        for i, j in restated.pair_order(K):
            value = fn(x[i], x[j], **kwargs)
            pairs[i, j] = value[metric] if isinstance(value, dict) else value
        got = (ens.ensemble_skill(x, o, metric, **kwargs), ens.ensemble_spread(x, metric, **kwargs), pairs)
        assert np.array_equal(np.mean([pairs[i, j] for i, j in restated.pair_order(K)]), got[1], equal_nan=True)
        want = (restated.ensemble_skill(x, o, metric, **kwargs), restated.ensemble_spread(x, metric, **kwargs),
                restated.pair_scores(x, metric, **kwargs))
        return got, want

    taken = []

    def measured(got, want):
        """The reference's deviation from the restatement; the values its own rounding took (NaN for a finite score) are
        counted, not measured."""
        gone = restated.lost(got, want)
        taken.append(int(gone.sum()))
        return restated.deviation(got, want, skip=gone)

    for name, K, (m, n), pattern in restated.CASES:
        x32, o32 = restated.members(K, m, n, 100 + len(name) + K, np.float32, pattern)
        out[name + "__x"], out[name + "__o"] = x32, o32
        for dtype in ("float32", "float64"):
            x, o = x32.astype(dtype), o32.astype(dtype)
            skill, spread, pairs, exact = [], [], [], []
            with warnings.catch_warnings(), np.errstate(all="ignore"):
                warnings.simplefilter("ignore")
                for label, metric, kwargs in metrics:
                    got, want = reference(x, o, metric, kwargs)
                    skill.append(got[0]), spread.append(got[1]), pairs.append(got[2])
                    if metric in restated.CAT_METRICS:
                        assert all(np.array_equal(g, w, equal_nan=True) for g, w in zip(got, want)), (name, dtype, label)
                    else:
                        key = "fss" if metric == "fss" else dtype
                        deviation[key] = max([deviation[key]] + [measured(g, w) for g, w in zip(got, want)])
                    exact.append(want)
                tables = []
                for thr in restated.CAT_THRESHOLDS:
                    rows = []
                    for i, j in restated.pair_order(K):
                        obj = cat.det_cat_fct_init(thr)
                        cat.det_cat_fct_accum(obj, x[i], x[j])
                        rows.append([int(obj[k]) for k in ("hits", "misses", "false_alarms", "correct_negatives")])
                    tables.append(rows)
                out["%s__%s__tables" % (name, dtype)] = np.array(tables, dtype=np.int64)
                if name == restated.CONDITIONED_CASE:
                    for c, (metric, kwargs) in enumerate(restated.CONDITIONED):
                        got, want = reference(x, o, metric, kwargs)
                        deviation[dtype] = max([deviation[dtype]] + [measured(g, w) for g, w in zip(got, want)])
                        tag = "%s__%s__cond_%d__" % (name, dtype, c)
                        out[tag + "skill"], out[tag + "spread"], out[tag + "pairs"] = np.float64(got[0]), np.float64(got[1]), got[2]
                        out[tag + "exact_skill"], out[tag + "exact_spread"] = np.float64(want[0]), np.float64(want[1])
                        out[tag + "exact_pairs"] = want[2]
            out["%s__%s__skill" % (name, dtype)] = np.array(skill, dtype=np.float64)
            out["%s__%s__spread" % (name, dtype)] = np.array(spread, dtype=np.float64)
            out["%s__%s__pairs" % (name, dtype)] = np.stack(pairs)
            out["%s__%s__exact_skill" % (name, dtype)] = np.array([e[0] for e in exact], dtype=np.float64)
            out["%s__%s__exact_spread" % (name, dtype)] = np.array([e[1] for e in exact], dtype=np.float64)
            out["%s__%s__exact_pairs" % (name, dtype)] = np.stack([e[2] for e in exact])

    x = out[restated.CONDITIONED_CASE + "__x"].astype(np.float64)
    o = out[restated.CONDITIONED_CASE + "__o"].astype(np.float64)
    messages = {}
    for key, call in (("skill_2d", lambda: ens.ensemble_skill(x[0], o, "RMSE")),
                      ("spread_2d", lambda: ens.ensemble_spread(x[0], "RMSE")),
                      ("spread_one_member", lambda: ens.ensemble_spread(x[:1], "RMSE")),
                      ("skill_shape", lambda: ens.ensemble_skill(x, o[:, :5], "RMSE")),
                      ("skill_lower_case", lambda: ens.ensemble_skill(x, o, "rmse")),
                      ("spread_lower_case", lambda: ens.ensemble_spread(x, "csi", thr=0.5)),
                      ("spread_unknown", lambda: ens.ensemble_spread(x, "no_such_score"))):
        try:
            call()
            raise AssertionError(key)
        except (ValueError, KeyError) as exc:
            messages[key] = [type(exc).__name__, str(exc)]
    out["messages"] = np.array(json.dumps(messages))
    out["reference_lost"] = np.int64(sum(taken))
    for key, value in deviation.items():
        out["deviation_" + key] = np.float64(value)
    np.savez_compressed(OUT, **out)
    print("%s: %d cases, %.1f KiB; the reference's scores deviate from the restatement by %.3g (float32 stacks), %.3g "
          "(float64 stacks) and %.3g (FSS), relative; %d results lost to the reference's own rounding"
          % (OUT, len(restated.CASES), os.path.getsize(OUT) / 1024.0, deviation["float32"], deviation["float64"], deviation["fss"],
             sum(taken)))


if __name__ == "__main__":
    main()
