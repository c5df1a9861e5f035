"""Golden vectors for the deterministic verification scores (``pysteps_amd.verification.detcatscores`` and
``detcontscores``), written by the UNMODIFIED reference.

    python tools/make_golden_detscores.py        (-> tests/golden/detscores_reference.npz)

Runs ``det_cat_fct_*`` and ``det_cont_fct_*`` of the reference package that ``oracle.build_ref`` prepares under
oracle/_ref.  Fields are stored as float32 (every value is a float32 number, so the float64 run uses the same numbers
widened).  Per case ``<case>__f`` and ``<case>__o``; per case and dtype

    <case>__<dtype>__counts          (nthr, 4[, K])  hits, misses, false alarms, correct negatives for ``thresholds``
    <case>__<dtype>__cat             (nthr, nscore[, K])  det_cat_fct_compute, scores in the order of ``cat_scores``
    <case>__<dtype>__<cond>__obj     (10[, K])  the error object: ``moments`` then ``n``, conditioning none/single/double
    <case>__<dtype>__<cond>__cont    (nscore[, K])  det_cont_fct_compute, scores in the order of ``cont_scores``

Cases, all 33 x 47: ``clean`` (no NaN: -1 is exceeded by every pixel, 1e6 by none, so every margin of the table is empty
once), ``nan_f``, ``nan_o``, ``nan_both`` (NaN in the forecast only, in the observation only, in both), ``flat`` (a
constant observation: its variance vanishes), ``members`` (a stack of 3 with ``axis=(1, 2)``).  ``merge__*``: object A
after two accumulations, object B after one, and the reference's merge of the two with its scores.  ``warnings`` holds the
texts NumPy raised in the two ``_compute`` functions per case, ``messages`` the texts of the reference's ValueErrors.
The continuous threshold is ``cont_thr``.  ``deviation_float32`` and ``deviation_float64`` are the largest relative deviations
of a moment of the reference's single-accumulation objects above (me, mse, mss, mae, mobs, mpred, vobs, vpred, cov) from
the longdouble evaluation of its definition (tests/helpers/detscores.py), per dtype of the fields; the GPU tests allow
5 x these.  Every conditioned case keeps at least three pairs (asserted here).  Needs the
reference; never runs on the GPU machine.
"""
import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUT = os.path.join(ROOT, "tests", "golden", "detscores_reference.npz")
M, N = 33, 47


def cases():
    from helpers import detscores as restated

    flat_f, _ = restated.pair(M, N, 15)
    members = [restated.pair(M, N, 20 + k, nan_f=0.02, nan_o=0.02 * (k % 2)) for k in range(3)]
    return [("clean", restated.pair(M, N, 11)), ("nan_f", restated.pair(M, N, 12, nan_f=0.03)),
            ("nan_o", restated.pair(M, N, 13, nan_o=0.03)), ("nan_both", restated.pair(M, N, 14, nan_f=0.0226, nan_o=0.0271)),
            ("flat", (flat_f, np.full((M, N), 1.0, np.float32))),
            ("members", (np.stack([p[0] for p in members]), np.stack([p[1] for p in members])))]


def caught(fn, *args):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        result = fn(*args)
    return result, sorted({str(w.message) for w in rec})


def cont_probe(cont):
    obj = cont.det_cont_fct_init()
    cont.det_cont_fct_accum(obj, np.eye(2), np.eye(2) + 1.0)
    return obj


def main():
    from helpers import detscores as restated
    from oracle import build_ref

    build_ref.build()
    build_ref.activate()
    from pysteps.verification import detcatscores as cat
    from pysteps.verification import detcontscores as cont

    thrs = restated.THRESHOLDS
    out = {"versions": np.array(json.dumps({"numpy": np.__version__})), "thresholds": np.array(thrs, dtype=np.float64),
           "cont_thr": np.float64(restated.CONT_THR), "cat_scores": np.array(restated.CAT_SCORES),
           "cont_scores": np.array(restated.CONT_SCORES), "moments": np.array(restated.MOMENTS),
           "cat_keys": np.array(sorted(cat.det_cat_fct_init(1.0))), "cont_keys": np.array(sorted(cont.det_cont_fct_init()))}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert list(cat.det_cat_fct(np.eye(2), np.eye(2) + 1.0, 0.5)) == restated.CAT_SCORES
        assert list(cont.det_cont_fct_compute(cont_probe(cont))) == restated.CONT_SCORES
    a23, a32, a234 = np.zeros((2, 3)), np.zeros((3, 2)), np.zeros((2, 3, 4))
    filled_cat, filled_cont = cat.det_cat_fct_init(1.0, axis=(1, 2)), cont.det_cont_fct_init(axis=(1, 2))
    cat.det_cat_fct_accum(filled_cat, a234, a234)
    cont.det_cont_fct_accum(filled_cont, a234 + 1.0, a234)
    messages = {}
    for key, call in (
            ("cat_shape", lambda: cat.det_cat_fct_accum(cat.det_cat_fct_init(1.0), a23, a32)),
            ("cat_axis", lambda: cat.det_cat_fct_accum(cat.det_cat_fct_init(1.0, axis=2), a23, a23)),
            ("cat_table", lambda: cat.det_cat_fct_accum(filled_cat, np.zeros((3, 3, 4)), np.zeros((3, 3, 4)))),
            ("cat_merge_thr", lambda: cat.det_cat_fct_merge(cat.det_cat_fct_init(1.0), cat.det_cat_fct_init(2.0))),
            ("cat_merge_axis", lambda: cat.det_cat_fct_merge(cat.det_cat_fct_init(1.0), cat.det_cat_fct_init(1.0, axis=0))),
            ("cat_merge_empty", lambda: cat.det_cat_fct_merge(cat.det_cat_fct_init(1.0), cat.det_cat_fct_init(1.0))),
            ("cont_shape", lambda: cont.det_cont_fct_accum(cont.det_cont_fct_init(), a23, a32)),
            ("cont_axis", lambda: cont.det_cont_fct_accum(cont.det_cont_fct_init(axis=2), a23, a23)),
            ("cont_object", lambda: cont.det_cont_fct_accum(filled_cont, np.zeros((3, 3, 4)), np.zeros((3, 3, 4)))),
            ("cont_conditioning", lambda: cont.det_cont_fct_accum(cont.det_cont_fct_init(conditioning="triple"), a23, a23)),
            ("cont_merge_axis", lambda: cont.det_cont_fct_merge(cont.det_cont_fct_init(), cont.det_cont_fct_init(axis=0))),
            ("cont_merge_conditioning", lambda: cont.det_cont_fct_merge(cont.det_cont_fct_init(),
                                                                        cont.det_cont_fct_init(conditioning="single"))),
            ("cont_merge_thr", lambda: cont.det_cont_fct_merge(cont.det_cont_fct_init(), cont.det_cont_fct_init(thr=1.0))),
            ("cont_merge_empty", lambda: cont.det_cont_fct_merge(cont.det_cont_fct_init(), cont.det_cont_fct_init()))):
        try:
            call()
            raise AssertionError(key)
        except ValueError as exc:
            messages[key] = str(exc)
    out["messages"] = np.array(json.dumps(messages))

    def cat_object(f, o, thr, axis):
        obj = cat.det_cat_fct_init(thr, axis)
        cat.det_cat_fct_accum(obj, f, o)
        return obj

    def cont_object(f, o, cond, axis):
        obj = cont.det_cont_fct_init(axis=axis, conditioning=cond, thr=restated.CONT_THR)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            cont.det_cont_fct_accum(obj, f, o)
        return obj

    def cont_array(obj):
        return np.stack([np.asarray(obj[k], dtype=np.float64) for k in restated.MOMENTS + ["n"]])

    names, seen, deviation = [], {}, {"float32": 0.0, "float64": 0.0}
    for name, (f32, o32) in cases():
        names.append(name)
        out[name + "__f"], out[name + "__o"] = f32, o32
        axis = (1, 2) if f32.ndim == 3 else None
        for dtype in ("float32", "float64"):
            f, o = f32.astype(dtype), o32.astype(dtype)
            tables, scores, said = [], [], set()
            for thr in thrs:
                obj = cat_object(f, o, thr, axis)
                assert obj["hits"].dtype == np.dtype(int)
                tables.append(np.stack([obj[k] for k in restated.CAT_KEYS]))
                result, texts = caught(cat.det_cat_fct_compute, obj)
                said |= set(texts)
                scores.append(np.stack([np.asarray(result[s], dtype=np.float64) for s in restated.CAT_SCORES]))
            assert np.all(np.sum(tables, axis=1) == M * N)
            out["%s__%s__counts" % (name, dtype)] = np.stack(tables)
            out["%s__%s__cat" % (name, dtype)] = np.stack(scores)
            seen["%s__%s__cat" % (name, dtype)] = sorted(said)
            for cond in restated.CONDITIONINGS:
                obj = cont_object(f, o, cond, axis)
                assert np.all(obj["n"] >= 3), (name, dtype, cond)
                result, texts = caught(cont.det_cont_fct_compute, obj)
                tag = "%s__%s__%s" % (name, dtype, cond or "none")
                out[tag + "__obj"] = cont_array(obj)
                deviation[dtype] = max(deviation[dtype], restated.reference_deviation(out[tag + "__obj"], f, o, cond))
                out[tag + "__cont"] = np.stack([np.asarray(result[s], dtype=np.float64) for s in restated.CONT_SCORES])
                seen[tag + "__cont"] = texts

    # two accumulations, then a merge
    pairs = [restated.pair(M, N, 31, nan_f=0.02), restated.pair(M, N, 32, nan_o=0.02), restated.pair(M, N, 33, nan_f=0.01, nan_o=0.01)]
    for i, (f32, o32) in enumerate(pairs):
        out["merge__f%d" % i], out["merge__o%d" % i] = f32, o32
    for dtype in ("float32", "float64"):
        typed = [(f.astype(dtype), o.astype(dtype)) for f, o in pairs]
        a, b = cat.det_cat_fct_init(thrs[1]), cat.det_cat_fct_init(thrs[1])
        cat.det_cat_fct_accum(a, *typed[0])
        cat.det_cat_fct_accum(a, *typed[1])
        cat.det_cat_fct_accum(b, *typed[2])
        out["merge__%s__cat_a" % dtype] = np.stack([a[k] for k in restated.CAT_KEYS])
        out["merge__%s__cat_b" % dtype] = np.stack([b[k] for k in restated.CAT_KEYS])
        merged = cat.det_cat_fct_merge(a, b)
        out["merge__%s__cat_merged" % dtype] = np.stack([merged[k] for k in restated.CAT_KEYS])
        result = cat.det_cat_fct_compute(merged)
        out["merge__%s__cat" % dtype] = np.stack([np.asarray(result[s], dtype=np.float64) for s in restated.CAT_SCORES])
        for cond in restated.CONDITIONINGS:
            a = cont.det_cont_fct_init(conditioning=cond, thr=restated.CONT_THR)
            b = cont.det_cont_fct_init(conditioning=cond, thr=restated.CONT_THR)
            cont.det_cont_fct_accum(a, *typed[0])
            tag = "merge__%s__%s" % (dtype, cond or "none")
            out[tag + "__first"] = cont_array(a)
            cont.det_cont_fct_accum(a, *typed[1])
            cont.det_cont_fct_accum(b, *typed[2])
            out[tag + "__a"], out[tag + "__b"] = cont_array(a), cont_array(b)
            merged = cont.det_cont_fct_merge(a, b)
            out[tag + "__merged"] = cont_array(merged)
            result = cont.det_cont_fct_compute(merged)
            out[tag + "__cont"] = np.stack([np.asarray(result[s], dtype=np.float64) for s in restated.CONT_SCORES])
    out["cases"] = np.array(names)
    out["deviation_float32"], out["deviation_float64"] = np.float64(deviation["float32"]), np.float64(deviation["float64"])
    out["warnings"] = np.array(json.dumps(seen))
    np.savez_compressed(OUT, **out)
    print("%s: %d cases, %.1f KiB; the reference's moments deviate from their definitions by %.3g (float32 fields) and %.3g "
          "(float64 fields), relative" % (OUT, len(names), os.path.getsize(OUT) / 1024.0, deviation["float32"], deviation["float64"]))


if __name__ == "__main__":
    main()
