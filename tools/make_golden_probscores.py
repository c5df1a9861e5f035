"""Golden vectors for the probabilistic verification scores (``pysteps_amd.verification.probscores``), written by the
UNMODIFIED reference.

    python tools/make_golden_probscores.py        (-> tests/golden/probscores_reference.npz)

Runs ``CRPS_*``, ``reldiag_*`` and ``ROC_curve_*`` of the reference package that ``oracle.build_ref`` prepares under
oracle/_ref.  Member and observation fields are stored as float32 (every value is a float32 number, so the float64 run
uses the same numbers widened), probability planes as float64 (the float32 run rounds them).

CRPS cases (``crps_cases``): ``<case>__f`` (K, m, n), ``<case>__o`` (m, n) and per dtype ``<case>__<dtype>__crps`` =
``[CRPS_sum, n, CRPS_compute]``.  ``ties_<K>`` are the nine pixels of tests/helpers/probscores.py ``tie_pixels``,
``quant_<K>`` 5 x 7 fields of four levels with NaN and +-inf in one member and in the observation, K in 1, 2, 3, 7, 20,
48, 64; ``rain_7`` a 33 x 65 gamma field; ``masked`` an observation of NaN only (n = 0: the reference's CRPS is NaN);
``twocalls`` the object after ``quant_3`` and then ``quant_7``.

Probability cases (``prob_cases``): ``<case>__p``, ``<case>__o``, and per dtype and number of bins (10 and 7)
``<case>__<dtype>__b<bins>__reldiag`` (4, bins) = X_sum, Y_sum, num_idx, sample_size and ``...__rf`` (2, bins) = r, f;
per dtype ``<case>__<dtype>__roc`` (4, 10) = hits, misses, false alarms, correct negatives, ``...__curve`` (2, 10) =
POFD, POD and ``...__area``.  ``k7`` holds probabilities j/7 over a 33 x 65 plane with NaN and +-inf on either side;
``edges`` holds the bin edges of both diagrams themselves, their float64 neighbours, 0.0, 1.0 and j/8, twelve times
each; ``mincount_a`` has nine pixels in bin 0, ten in bin 1 and thirty in bin 2; ``mincount_ab`` is the object after a
second call with ten pixels in bin 0, nine in bin 1 and eleven in bin 9.  ``x_min``, ``edges_b10``, ``edges_b7`` and
``prob_thrs`` are the reference's.

``deviation_float32`` and ``deviation_float64`` are the largest relative deviations of the reference's ``CRPS_sum`` and
``X_sum`` from the restated rule (tests/helpers/probscores.py: ``crps_exact`` in numpy.longdouble and ``crps_terms`` by
``math.fsum`` over float64 terms, whichever lies farther; the bins' sums by ``math.fsum``), per dtype of the fields; the GPU tests allow 5 x these.  Needs the reference; never runs on the GPU machine.
"""
import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUT = os.path.join(ROOT, "tests", "golden", "probscores_reference.npz")
X_MIN = 0.5
DTYPES = ("float32", "float64")
BINS = (10, 7)


def crps_cases():
    from helpers import probscores as restated

    cases = []
    for K in restated.MEMBER_COUNTS:
        cases.append(("ties_%d" % K, restated.tie_pixels(K)))
        cases.append(("quant_%d" % K, restated.ensemble(K, 5, 7, 100 + K, bad=True)))
    cases.append(("rain_7", restated.ensemble(7, 33, 65, 200, ties=False, bad=True)))
    members, obs = restated.ensemble(3, 5, 7, 300)
    cases.append(("masked", (members, np.full_like(obs, np.nan))))
    return cases


def prob_cases(edges):
    from helpers import probscores as restated

    p = restated.probabilities(7, (33, 65), 400)
    o = restated.rainy((33, 65), 401)
    for pixel, value in enumerate((np.nan, np.inf, -np.inf)):
        p.reshape(-1)[pixel] = value
        o.reshape(-1)[10 + pixel] = value
    values = [0.0, 1.0] + [j / 8.0 for j in range(9)]
    for e in edges:
        for x in e:
            values += [x, np.nextafter(x, np.inf), np.nextafter(x, -np.inf)]
    on_edges = np.tile(np.array(values, dtype=np.float64), (12, 1))
    a = np.array([0.05] * 9 + [0.15] * 10 + [0.25] * 30, dtype=np.float64).reshape(7, 7)
    b = np.array([0.05] * 10 + [0.15] * 9 + [0.95] * 11, dtype=np.float64).reshape(5, 6)
    return [("k7", p, o), ("edges", on_edges, restated.rainy(on_edges.shape, 402)), ("mincount_a", a, restated.rainy(a.shape, 403)),
            ("mincount_b", b, restated.rainy(b.shape, 404))]


def relative(got, exact):
    """|exact - got| / |got| in float64, as the tests form it against the stored value."""
    got, exact = np.float64(got), np.float64(exact)
    if got == 0:
        assert exact == 0
        return 0.0
    return float(abs(exact - got) / abs(got))


def main():
    from helpers import probscores as restated
    from oracle import build_ref

    build_ref.build()
    build_ref.activate()
    from pysteps.verification import probscores as ref

    edges = {n: ref.reldiag_init(X_MIN, n)["bin_edges"] for n in BINS}
    out = {"versions": np.array(json.dumps({"numpy": np.__version__})), "x_min": np.float64(X_MIN),
           "prob_thrs": ref.ROC_curve_init(X_MIN)["prob_thrs"], "crps_keys": np.array(sorted(ref.CRPS_init())),
           "reldiag_keys": np.array(sorted(ref.reldiag_init(X_MIN))), "roc_keys": np.array(sorted(ref.ROC_curve_init(X_MIN)))}
    for n in BINS:
        out["edges_b%d" % n] = edges[n]
    deviation = dict.fromkeys(DTYPES, 0.0)

    def crps_row(obj):
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            return np.array([obj["CRPS_sum"], obj["n"], ref.CRPS_compute(obj)], dtype=np.float64)

    names = []
    for name, (f32, o32) in crps_cases():
        names.append(name)
        out[name + "__f"], out[name + "__o"] = f32, o32
        for dtype in DTYPES:
            f, o = f32.astype(dtype), o32.astype(dtype)
            obj = ref.CRPS_init()
            ref.CRPS_accum(obj, f, o)
            assert isinstance(obj["n"], float) and np.array_equal(f, f32.astype(dtype), equal_nan=True)
            out["%s__%s__crps" % (name, dtype)] = crps_row(obj)
            n, exact = restated.crps_exact(f, o)
            assert n == int(obj["n"]), (name, dtype)
            deviation[dtype] = max(deviation[dtype], relative(obj["CRPS_sum"], exact), relative(obj["CRPS_sum"], restated.crps_terms(f, o)[1]))
    for dtype in DTYPES:
        obj = ref.CRPS_init()
        for name in ("quant_3", "quant_7"):
            ref.CRPS_accum(obj, out[name + "__f"].astype(dtype), out[name + "__o"].astype(dtype))
        out["twocalls__%s__crps" % dtype] = crps_row(obj)
    out["crps_cases"] = np.array(names)

    def reldiag_arrays(obj):
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            return (np.stack([np.asarray(obj[k], dtype=np.float64) for k in restated.BIN_KEYS]),
                    np.stack([np.asarray(v, dtype=np.float64) for v in ref.reldiag_compute(obj)]))

    def roc_arrays(obj):
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            pofd, pod, area = ref.ROC_curve_compute(obj, compute_area=True)
        return np.stack([obj[k] for k in restated.ROC_KEYS]), np.array([pofd, pod], dtype=np.float64), np.float64(area)

    names = []
    held = {}
    for name, p64, o32 in prob_cases([edges[n] for n in BINS]):
        names.append(name)
        out[name + "__p"], out[name + "__o"] = p64, o32
        for dtype in DTYPES:
            p, o = p64.astype(dtype), o32.astype(dtype)
            for n in BINS:
                obj = ref.reldiag_init(X_MIN, n)
                ref.reldiag_accum(obj, p, o)
                held[name, dtype, n] = obj
                tag = "%s__%s__b%d" % (name, dtype, n)
                out[tag + "__reldiag"], out[tag + "__rf"] = reldiag_arrays(obj)
                counted = restated.bin_counts(p, o, X_MIN, edges=edges[n])
                assert [c if c >= 10 else 0 for c in counted["count"]] == list(obj["num_idx"]), tag
                for b in range(n):
                    if counted["count"][b] >= 10:
                        deviation[dtype] = max(deviation[dtype], relative(obj["X_sum"][b], counted["sum"][b]))
            roc = ref.ROC_curve_init(X_MIN)
            ref.ROC_curve_accum(roc, p, o)
            held[name, dtype, "roc"] = roc
            tag = "%s__%s" % (name, dtype)
            out[tag + "__roc"], out[tag + "__curve"], out[tag + "__area"] = roc_arrays(roc)
            assert restated.bin_counts(p, o, X_MIN, prob_thrs=roc["prob_thrs"])["roc"] == out[tag + "__roc"].T.tolist(), tag
    # the second call of the min_count pair goes into the objects of the first
    for dtype in DTYPES:
        p, o = out["mincount_b__p"].astype(dtype), out["mincount_b__o"].astype(dtype)
        for n in BINS:
            obj = held["mincount_a", dtype, n]
            ref.reldiag_accum(obj, p, o)
            tag = "mincount_ab__%s__b%d" % (dtype, n)
            out[tag + "__reldiag"], out[tag + "__rf"] = reldiag_arrays(obj)
        roc = held["mincount_a", dtype, "roc"]
        ref.ROC_curve_accum(roc, p, o)
        out["mincount_ab__%s__roc" % dtype], out["mincount_ab__%s__curve" % dtype], out["mincount_ab__%s__area" % dtype] = roc_arrays(roc)
    first = out["mincount_a__float64__b10__reldiag"]
    assert first[2, 0] == 0 and first[2, 1] == 10 and first[2, 2] == 30  # nine pixels add nothing, ten add their sums
    both = out["mincount_ab__float64__b10__reldiag"]
    assert both[2, 0] == 10 and both[2, 1] == 10 and both[2, 9] == 11
    out["prob_cases"] = np.array(names)
    for dtype in DTYPES:
        assert deviation[dtype] > 0.0
        out["deviation_" + dtype] = np.float64(deviation[dtype])
    np.savez_compressed(OUT, **out)
    print("%s: %d CRPS cases, %d probability cases, %.1f KiB; the reference's CRPS_sum and X_sum deviate from the restated "
          "rule by %.3g (float32 fields) and %.3g (float64 fields), relative"
          % (OUT, len(out["crps_cases"]), len(names), os.path.getsize(OUT) / 1024.0, deviation["float32"], deviation["float64"]))


if __name__ == "__main__":
    main()
