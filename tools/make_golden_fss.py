"""Golden vectors for the fractions skill score (``pysteps_amd.verification.spatialscores``), written by the UNMODIFIED
reference.

    python tools/make_golden_fss.py        (-> tests/golden/fss_reference.npz)

Runs pysteps/verification/spatialscores.py ``fss_init`` / ``fss_accum`` / ``fss_compute`` of the reference package that
``oracle.build_ref`` prepares under oracle/_ref.  Per case the file holds the forecast ``<case>__f`` and the observation
``<case>__o`` as float32 (every value is a float32 number, so the float64 run uses the same numbers widened), and per
dtype the reference's three sums ``<case>__<dtype>__sums`` (nthr, nsc, 3: sum_fct_sq, sum_fct_obs, sum_obs_sq) and its
scores ``<case>__<dtype>__fss`` (nthr, nsc), for ``thresholds`` (Python floats) and ``scales``; ``keys`` are the keys of
the reference's FSS object and ``messages`` the texts of its three ValueErrors.

Cases: 257 x 311, 640 x 710 and 1024 x 1024 pairs of rain-like fields (tests/helpers/fss.py: NaN speckle, +inf and -inf
blocks, pixels exactly float32(0.7) against the threshold 0.7), an all-dry pair (the score is NaN) and a pair of
identical fields (the score is exactly 1).

The reference filters in floating point; the sums are integers over scale**4.  The script measures how far the
reference is from them (tests/helpers/fss.py counts the integers): ``deviation_sums``, the largest relative deviation of
a sum, and ``deviation_fss``, the largest absolute deviation of a score, over all cases above.  The tests allow 5 x
these.  Needs the reference; never runs on the GPU machine.
"""
import json
import os
import sys
import warnings
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUT = os.path.join(ROOT, "tests", "golden", "fss_reference.npz")


def cases():
    from helpers import fss as restated

    out = [("p257x311", restated.pair(257, 311, 1)), ("p640x710", restated.pair(640, 710, 2)),
           ("p1024x1024", restated.pair(1024, 1024, 3))]
    out.append(("dry64x80", (np.zeros((64, 80), np.float32), np.zeros((64, 80), np.float32))))
    same = restated.field(129, 140, 4)
    out.append(("same129x140", (same, same.copy())))
    return out


def main():
    import scipy

    from helpers import fss as restated
    from oracle import build_ref

    build_ref.build()
    build_ref.activate()
    from pysteps.verification import spatialscores as ref

    thresholds, scales = restated.THRESHOLDS, restated.SCALES
    out = {"versions": np.array(json.dumps({"numpy": np.__version__, "scipy": scipy.__version__})),
           "thresholds": np.array(thresholds, dtype=np.float64), "scales": np.array(scales, dtype=np.int64),
           "keys": np.array(sorted(ref.fss_init(1.0, 2)))}
    messages = {}
    for key, call in (("shape", lambda: ref.fss_accum(ref.fss_init(1.0, 2), np.zeros((4, 5)), np.zeros((5, 4)))),
                      ("merge_thr", lambda: ref.fss_merge(ref.fss_init(1.0, 2), ref.fss_init(2.0, 2))),
                      ("merge_scale", lambda: ref.fss_merge(ref.fss_init(1.0, 2), ref.fss_init(1.0, 4)))):
        try:
            call()
        except ValueError as exc:
            messages[key] = str(exc)
    out["messages"] = np.array(json.dumps(messages))
    names, dev_sums, dev_fss = [], 0.0, 0.0
    for name, (f32, o32) in cases():
        names.append(name)
        out[name + "__f"], out[name + "__o"] = f32, o32
        for dtype in ("float32", "float64"):
            f, o = f32.astype(dtype), o32.astype(dtype)
            sums = np.empty((len(thresholds), len(scales), 3), dtype=np.float64)
            scores = np.empty((len(thresholds), len(scales)), dtype=np.float64)
            exact = restated.sums_table(f, o, thresholds, scales)
            for i, thr in enumerate(thresholds):
                for j, scale in enumerate(scales):
                    obj = ref.fss_init(thr, scale)
                    ref.fss_accum(obj, f.copy(), o.copy())
                    with warnings.catch_warnings(), np.errstate(all="ignore"):
                        warnings.simplefilter("ignore")
                        scores[i, j] = ref.fss_compute(obj)
                    sums[i, j] = [obj["sum_fct_sq"], obj["sum_fct_obs"], obj["sum_obs_sq"]]
                    for got, count in zip(sums[i, j], exact[i, j]):
                        want = Fraction(int(count), restated.window(scale) ** 4)
                        if want == 0:
                            assert got == 0.0, (name, dtype, thr, scale)
                        else:
                            dev_sums = max(dev_sums, float(abs(Fraction(float(got)) - want) / want))
                    want = restated.score(exact[i, j], scale)
                    assert np.isnan(want) == np.isnan(scores[i, j]), (name, dtype, thr, scale)
                    if not np.isnan(want):
                        dev_fss = max(dev_fss, abs(float(scores[i, j]) - float(want)))
            out["%s__%s__sums" % (name, dtype)] = sums
            out["%s__%s__fss" % (name, dtype)] = scores
    out["cases"] = np.array(names)
    out["deviation_sums"], out["deviation_fss"] = np.float64(dev_sums), np.float64(dev_fss)
    np.savez_compressed(OUT, **out)
    print("%s: %d cases, %.1f KiB; the reference deviates from the exact integers by %.3g (relative, sums) and %.3g "
          "(absolute, FSS)" % (OUT, len(names), os.path.getsize(OUT) / 1024.0, dev_sums, dev_fss))


if __name__ == "__main__":
    main()
