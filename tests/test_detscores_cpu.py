"""The deterministic verification scores' host side (no GPU): the restatement of tests/helpers/detscores.py against the
reference's goldens, the host arithmetic (``_merge``, ``_compute``) bit for bit, and the Python layer (objects, messages,
fall-back, accumulator, registration) with the restatement standing in for the kernels.

Yardstick for the continuous moments: the reference's own error.  tools/make_golden_detscores.py measured every moment
of the reference's single-accumulation objects (me, mse, mss, mae, mobs, mpred, vobs, vpred, cov; all cases and
conditionings of tests/golden/detscores_reference.npz) against the longdouble evaluation of its definition.  Largest
relative deviation: 9.73e-07 for float32 fields (the reference forms residuals, squares and means in float32) and
6.8e-15 for float64 fields.  ``test_reference_deviation_is_the_recorded_one`` measures them again.  The GPU tests allow
5 x these (4.9e-06 and 3.4e-14), the project's standing rule; contingency counts and categorical scores have no
tolerance.
"""

import json
import os
import warnings

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import detscores as restated

PATH = os.path.join(GOLDEN, "detscores_reference.npz")
DTYPES = ["float32", "float64"]
CONDS = [(None, "none"), ("single", "single"), ("double", "double")]


@pytest.fixture(scope="module")
def golden():
    return np.load(PATH)


def case_names():
    return [str(c) for c in np.load(PATH)["cases"]]


def thresholds_of(golden):
    return [float(t) for t in golden["thresholds"]]  # Python floats, as the golden run used


def cont_object(array, axis=None, conditioning=None, thr=restated.CONT_THR):
    """The error object behind a golden array (10,) or (10, K)."""
    obj = {"axis": axis, "conditioning": conditioning, "thr": thr}
    for i, key in enumerate(restated.MOMENTS + ["n"]):
        obj[key] = np.array(array[i], dtype=np.float64)
    return obj


def cat_object(array, thr, axis=None):
    obj = {"thr": thr, "axis": axis}
    for i, key in enumerate(restated.CAT_KEYS):
        obj[key] = np.array(array[i], dtype=int)
    return obj


def as_array(obj):
    return np.stack([np.asarray(obj[k], dtype=np.float64) for k in restated.MOMENTS + ["n"]])


def scores_array(result, names):
    return np.stack([np.asarray(result[s], dtype=np.float64) for s in names])


def caught(fn, *args):
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        result = fn(*args)
    return result, sorted({str(w.message) for w in rec})


def within(got, want, bar):
    """NaN positions equal, infinities equal, everything else within ``bar`` relative."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
    worst = float(np.max(np.abs(got[fin] - want[fin]) / np.where(want[fin] == 0, 1.0, np.abs(want[fin])), initial=0.0))
    assert np.all(got[fin][want[fin] == 0] == 0.0)
    assert worst <= bar, (worst, bar)
    return worst


@pytest.fixture
def host_kernel(monkeypatch):
    """The Python layer with tests/helpers/detscores.py in place of the two entry points: fields stay NumPy arrays,
    thresholds arrive as the float64 numbers to compare with."""
    from pysteps_amd.verification import detcatscores, detcontscores, detscores

    def fields(dev_f, dev_o, K, npix, shared):
        f = np.asarray(dev_f, dtype=np.float64).reshape(K, npix)
        o = np.asarray(dev_o, dtype=np.float64).reshape((1, npix) if shared else (K, npix))
        return f, (np.broadcast_to(o, (K, npix)) if shared else o)

    def counts(dev_f, dev_o, K, npix, shared, thr_f, thr_o):
        f, o = fields(dev_f, dev_o, K, npix, shared)
        out = np.empty((K, len(thr_f), 4), dtype=np.uint64)
        for k in range(K):
            for i, (tf, to) in enumerate(zip(thr_f, thr_o)):
                with np.errstate(invalid="ignore"):
                    pb, ob = f[k] > np.float64(tf), o[k] > np.float64(to)
                out[k, i] = [(pb & ob).sum(), (~pb & ob).sum(), (pb & ~ob).sum(), (~pb & ~ob).sum()]
        return out

    def sums(dev_f, dev_o, K, npix, shared, conditioning, thr_f, thr_o):
        f, o = fields(dev_f, dev_o, K, npix, shared)
        cnt, out = np.zeros((K, 4), dtype=np.uint64), np.zeros((K, 11, 2), dtype=np.float64)
        for k in range(K):
            p, q = f[k].copy(), o[k].copy()
            cnt[k, 3] = np.isinf(p).sum() + np.isinf(q).sum()
            if conditioning:
                with np.errstate(invalid="ignore"):
                    pb, ob = p > thr_f, q > thr_o
                keep = (pb | ob) if conditioning == 1 else (pb & ob)
                p[~keep] = np.nan
                q[~keep] = np.nan
            p[np.isinf(p)] = np.nan  # the stand-in leaves infinite values out; the layer declines on the count
            q[np.isinf(q)] = np.nan
            c, s, _ = restated.raw_sums(p, q)
            cnt[k, :3] = c
            out[k, :, 0] = [s[name] for name in restated.SUMS]
        return cnt, out

    monkeypatch.setattr(detcatscores, "_counts", counts)
    monkeypatch.setattr(detcontscores, "_sums", sums)
    monkeypatch.setattr(detcatscores, "_upload", lambda X: np.asarray(X))
    monkeypatch.setattr(detcontscores, "_upload", lambda X: np.asarray(X))
    return detcatscores, detcontscores, detscores


def test_golden_covers_the_required_cases(golden):
    assert case_names() == ["clean", "nan_f", "nan_o", "nan_both", "flat", "members"]
    assert golden["clean__f"].shape == (33, 47) and golden["clean__f"].dtype == np.float32 and 33 * 47 % 4 == 3
    nan = {name: (bool(np.isnan(golden[name + "__f"]).any()), bool(np.isnan(golden[name + "__o"]).any())) for name in case_names()}
    assert nan["clean"] == (False, False) and nan["nan_f"] == (True, False) and nan["nan_o"] == (False, True)
    assert nan["nan_both"] == (True, True) and golden["members__f"].shape == (3, 33, 47)
    counts = golden["clean__float64__counts"]  # (nthr, 4): no pixel exceeds 1e6, every pixel exceeds -1
    assert list(counts[2]) == [0, 0, 0, 1551] and list(counts[3]) == [1551, 0, 0, 0]
    assert np.isnan(golden["clean__float64__cat"][2]).any() and np.isnan(golden["clean__float64__cat"][3]).any()
    assert json.loads(str(golden["warnings"]))["clean__float64__cat"]  # the zero divisions warned
    assert golden["flat__float64__none__obj"][1] == 0.0 and not np.isfinite(golden["flat__float64__none__cont"]).all()
    for name in case_names():
        for dtype in DTYPES:
            for _, tag in CONDS:
                assert np.all(golden["%s__%s__%s__obj" % (name, dtype, tag)][9] >= 3)
    assert 0.0 < float(golden["deviation_float64"]) < 1e-13 < float(golden["deviation_float32"]) < 1e-5


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", case_names())
def test_restatement_reproduces_every_golden_count(golden, name, dtype):
    f, o = golden[name + "__f"].astype(dtype), golden[name + "__o"].astype(dtype)
    want = golden["%s__%s__counts" % (name, dtype)]
    for i, thr in enumerate(thresholds_of(golden)):
        if f.ndim == 3:
            for k in range(f.shape[0]):
                assert list(restated.counts(f[k], o[k], thr)) == [int(c) for c in want[i, :, k]]
        else:
            assert list(restated.counts(f, o, thr)) == [int(c) for c in want[i]]
    for cond, tag in CONDS:
        obj = golden["%s__%s__%s__obj" % (name, dtype, tag)]
        stack = zip(f, o) if f.ndim == 3 else [(f, o)]
        for k, (fk, ok) in enumerate(stack):
            assert restated.raw_sums(fk, ok, cond, restated.CONT_THR)[0][2] == int(obj[9, k] if f.ndim == 3 else obj[9])


def test_reference_deviation_is_the_recorded_one(golden):
    """The bar of the GPU tests: the reference's deviation from the longdouble definitions, per dtype of the fields."""
    worst = {"float32": 0.0, "float64": 0.0}
    for name in case_names():
        for dtype in DTYPES:
            f, o = golden[name + "__f"].astype(dtype), golden[name + "__o"].astype(dtype)
            for cond, tag in CONDS:
                worst[dtype] = max(worst[dtype], restated.reference_deviation(golden["%s__%s__%s__obj" % (name, dtype, tag)], f, o, cond))
    print("the reference's moments deviate by %.3g (float32 fields) and %.3g (float64 fields), relative" % (worst["float32"], worst["float64"]))
    assert worst["float32"] == float(golden["deviation_float32"]) and worst["float64"] == float(golden["deviation_float64"])
    assert abs(worst["float32"] - 9.73e-07) < 1e-9 and abs(worst["float64"] - 6.8e-15) < 1e-16  # the module docstring's


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", case_names())
def test_compute_returns_the_references_bits(golden, name, dtype):
    from pysteps_amd.verification import detcatscores, detcontscores

    said = json.loads(str(golden["warnings"]))
    texts = set()
    for i, thr in enumerate(thresholds_of(golden)):
        result, new = caught(detcatscores.det_cat_fct_compute, cat_object(golden["%s__%s__counts" % (name, dtype)][i], thr))
        texts |= set(new)
        assert list(result) == restated.CAT_SCORES
        np.testing.assert_array_equal(scores_array(result, restated.CAT_SCORES), golden["%s__%s__cat" % (name, dtype)][i])
    assert sorted(texts) == said["%s__%s__cat" % (name, dtype)]
    for cond, tag in CONDS:
        key = "%s__%s__%s" % (name, dtype, tag)
        result, new = caught(detcontscores.det_cont_fct_compute, cont_object(golden[key + "__obj"], conditioning=cond))
        assert list(result) == restated.CONT_SCORES and new == said[key + "__cont"]
        np.testing.assert_array_equal(scores_array(result, restated.CONT_SCORES), golden[key + "__cont"])
    one = detcontscores.det_cont_fct_compute(cont_object(golden["%s__%s__none__obj" % (name, dtype)]), ["RMSE", "pearsonr", None, "ets"])
    assert list(one) == ["RMSE", "corr_p"]
    ets = detcatscores.det_cat_fct_compute(cat_object(golden["%s__%s__counts" % (name, dtype)][0], 0.5), ["ets", "gss", None])
    assert list(ets) == ["ETS", "GSS"] and np.array_equal(ets["ETS"], ets["GSS"], equal_nan=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_merge_returns_the_references_bits(golden, dtype):
    from pysteps_amd.verification import detcatscores, detcontscores

    thr = thresholds_of(golden)[1]
    a, b = cat_object(golden["merge__%s__cat_a" % dtype], thr), cat_object(golden["merge__%s__cat_b" % dtype], thr)
    merged = detcatscores.det_cat_fct_merge(a, b)
    assert merged["hits"].dtype == np.dtype(int) and merged["hits"] is a["hits"]  # the reference's shallow copy
    np.testing.assert_array_equal(np.stack([merged[k] for k in restated.CAT_KEYS]), golden["merge__%s__cat_merged" % dtype])
    np.testing.assert_array_equal(scores_array(detcatscores.det_cat_fct_compute(merged), restated.CAT_SCORES),
                                  golden["merge__%s__cat" % dtype])
    for cond, tag in CONDS:
        key = "merge__%s__%s" % (dtype, tag)
        a, b = cont_object(golden[key + "__a"], conditioning=cond), cont_object(golden[key + "__b"], conditioning=cond)
        merged = detcontscores.det_cont_fct_merge(a, b)
        np.testing.assert_array_equal(as_array(merged), golden[key + "__merged"])
        np.testing.assert_array_equal(as_array(b), golden[key + "__b"])
        np.testing.assert_array_equal(scores_array(detcontscores.det_cont_fct_compute(merged), restated.CONT_SCORES),
                                      golden[key + "__cont"])


def test_objects_and_messages_equal_the_references(golden):
    from pysteps_amd.verification import detcatscores as cat
    from pysteps_amd.verification import detcontscores as cont

    assert sorted(cat.det_cat_fct_init(1.0)) == [str(k) for k in golden["cat_keys"]]
    assert sorted(cont.det_cont_fct_init()) == [str(k) for k in golden["cont_keys"]]
    assert cat.det_cat_fct_init(1.0, axis=2)["axis"] == (2,) and cat.det_cat_fct_init(1.0, axis=[1, 2])["axis"] == [1, 2]
    assert cont.det_cont_fct_init(axis=0)["axis"] == (0,) and cont.det_cont_fct_init()["axis"] is None
    assert all(v is None for k, v in cont.det_cont_fct_init().items() if k not in ("axis", "conditioning", "thr"))
    a23, a32 = np.zeros((2, 3)), np.zeros((3, 2))
    filled_cat = cat_object(np.zeros((4, 2), dtype=int), 1.0, axis=(1, 2))
    filled_cont = cont_object(np.zeros((10, 2)), axis=(1, 2), thr=0.0)
    calls = {
        "cat_shape": lambda: cat.det_cat_fct_accum(cat.det_cat_fct_init(1.0), a23, a32),
        "cat_axis": lambda: cat.det_cat_fct_accum(cat.det_cat_fct_init(1.0, axis=2), a23, a23),
        "cat_table": lambda: cat.det_cat_fct_accum(filled_cat, np.zeros((3, 3, 4)), np.zeros((3, 3, 4))),
        "cat_merge_thr": lambda: cat.det_cat_fct_merge(cat.det_cat_fct_init(1.0), cat.det_cat_fct_init(2.0)),
        "cat_merge_axis": lambda: cat.det_cat_fct_merge(cat.det_cat_fct_init(1.0), cat.det_cat_fct_init(1.0, axis=0)),
        "cat_merge_empty": lambda: cat.det_cat_fct_merge(cat.det_cat_fct_init(1.0), cat.det_cat_fct_init(1.0)),
        "cont_shape": lambda: cont.det_cont_fct_accum(cont.det_cont_fct_init(), a23, a32),
        "cont_axis": lambda: cont.det_cont_fct_accum(cont.det_cont_fct_init(axis=2), a23, a23),
        "cont_object": lambda: cont.det_cont_fct_accum(filled_cont, np.zeros((3, 3, 4)), np.zeros((3, 3, 4))),
        "cont_conditioning": lambda: cont.det_cont_fct_accum(cont.det_cont_fct_init(conditioning="triple"), a23, a23),
        "cont_merge_axis": lambda: cont.det_cont_fct_merge(cont.det_cont_fct_init(), cont.det_cont_fct_init(axis=0)),
        "cont_merge_conditioning": lambda: cont.det_cont_fct_merge(cont.det_cont_fct_init(), cont.det_cont_fct_init(conditioning="single")),
        "cont_merge_thr": lambda: cont.det_cont_fct_merge(cont.det_cont_fct_init(), cont.det_cont_fct_init(thr=1.0)),
        "cont_merge_empty": lambda: cont.det_cont_fct_merge(cont.det_cont_fct_init(), cont.det_cont_fct_init()),
    }
    messages = json.loads(str(golden["messages"]))
    assert sorted(calls) == sorted(messages)
    for key, call in calls.items():
        with pytest.raises(ValueError) as exc:
            call()
        assert str(exc.value) == messages[key], key


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", case_names())
def test_python_layer_scores_the_goldens(golden, host_kernel, name, dtype):
    """_accum, the public functions and the tables through the restated kernels: counts and categorical scores with no
    tolerance, moments and continuous scores within the GPU bar."""
    cat, cont, _ = host_kernel
    bar = 5.0 * float(golden["deviation_" + dtype])
    f, o = golden[name + "__f"].astype(dtype), golden[name + "__o"].astype(dtype)
    axis = (1, 2) if f.ndim == 3 else None
    thrs = thresholds_of(golden)
    for i, thr in enumerate(thrs):
        obj = cat.det_cat_fct_init(thr, axis)
        cat.det_cat_fct_accum(obj, f, o)
        assert all(obj[k].dtype == np.dtype(int) and obj[k].shape == f.shape[:-2] * (f.ndim == 3) for k in restated.CAT_KEYS)
        np.testing.assert_array_equal(np.stack([obj[k] for k in restated.CAT_KEYS]), golden["%s__%s__counts" % (name, dtype)][i])
        with np.errstate(all="ignore"):
            np.testing.assert_array_equal(scores_array(cat.det_cat_fct(f, o, thr, axis=axis), restated.CAT_SCORES),
                                          golden["%s__%s__cat" % (name, dtype)][i])
    with np.errstate(all="ignore"):
        table, counts = cat.det_cat_table(f, o, thrs, return_counts=True)
    want = golden["%s__%s__cat" % (name, dtype)]  # (nthr, nscore[, K])
    np.testing.assert_array_equal(scores_array(table, restated.CAT_SCORES), np.moveaxis(want, 0, -1))
    assert counts.dtype == np.uint64 and counts.shape == f.shape[:-2] * (f.ndim == 3) + (len(thrs), 4)
    worst = 0.0
    for cond, tag in CONDS:
        key = "%s__%s__%s" % (name, dtype, tag)
        obj = cont.det_cont_fct_init(axis=axis, conditioning=cond, thr=restated.CONT_THR)
        cont.det_cont_fct_accum(obj, f, o)
        assert all(obj[k].dtype == np.float64 and obj[k].shape == golden[key + "__obj"].shape[1:] for k in restated.MOMENTS + ["n"])
        worst = max(worst, within(as_array(obj), golden[key + "__obj"], bar))
        with np.errstate(all="ignore"):
            online = cont.det_cont_fct(f, o, restated.CONT_SCORES, axis=axis, conditioning=cond, thr=restated.CONT_THR)
            table = cont.det_cont_table(f, o, cond, restated.CONT_THR)
        worst = max(worst, within(scores_array(online, restated.CONT_SCORES), golden[key + "__cont"], bar))
        np.testing.assert_array_equal(scores_array(table, restated.CONT_SCORES), scores_array(online, restated.CONT_SCORES))
    print("%s %s: moments and continuous scores within %.3g of the golden (bar %.3g)" % (name, dtype, worst, bar))


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_accumulations_and_a_merge(golden, host_kernel, dtype):
    cat, cont, _ = host_kernel
    bar = 5.0 * float(golden["deviation_" + dtype])
    pairs = [(golden["merge__f%d" % i].astype(dtype), golden["merge__o%d" % i].astype(dtype)) for i in range(3)]
    thr = thresholds_of(golden)[1]
    a, b = cat.det_cat_fct_init(thr), cat.det_cat_fct_init(thr)
    cat.det_cat_fct_accum(a, *pairs[0])
    cat.det_cat_fct_accum(a, *pairs[1])
    cat.det_cat_fct_accum(b, *pairs[2])
    np.testing.assert_array_equal(np.stack([a[k] for k in restated.CAT_KEYS]), golden["merge__%s__cat_a" % dtype])
    merged = cat.det_cat_fct_merge(a, b)
    np.testing.assert_array_equal(np.stack([merged[k] for k in restated.CAT_KEYS]), golden["merge__%s__cat_merged" % dtype])
    for cond, tag in CONDS:
        key = "merge__%s__%s" % (dtype, tag)
        a = cont.det_cont_fct_init(conditioning=cond, thr=restated.CONT_THR)
        b = cont.det_cont_fct_init(conditioning=cond, thr=restated.CONT_THR)
        cont.det_cont_fct_accum(a, *pairs[0])
        within(as_array(a), golden[key + "__first"], bar)
        cont.det_cont_fct_accum(a, *pairs[1])
        cont.det_cont_fct_accum(b, *pairs[2])
        within(as_array(a), golden[key + "__a"], bar)
        merged = cont.det_cont_fct_merge(a, b)
        within(as_array(merged), golden[key + "__merged"], bar)
        within(scores_array(cont.det_cont_fct_compute(merged), restated.CONT_SCORES), golden[key + "__cont"], bar)
        # an all-NaN batch leaves the object untouched, as in the reference
        before = as_array(merged)
        with pytest.warns(RuntimeWarning):
            cont.det_cont_fct_accum(merged, np.full((5, 7), np.nan, dtype), np.zeros((5, 7), dtype))
        np.testing.assert_array_equal(as_array(merged), before)


def test_objects_interchange_with_the_references(golden, host_kernel, ref_pysteps):
    from pysteps.verification import detcatscores as ref_cat
    from pysteps.verification import detcontscores as ref_cont

    cat, cont, _ = host_kernel
    bar = 5.0 * float(golden["deviation_float64"])
    (f0, o0), (f1, o1) = [(golden["merge__f%d" % i].astype(np.float64), golden["merge__o%d" % i].astype(np.float64)) for i in (0, 1)]
    mine, theirs = cat.det_cat_fct_init(1.0), ref_cat.det_cat_fct_init(1.0)
    assert mine == theirs
    cat.det_cat_fct_accum(mine, f0, o0)
    ref_cat.det_cat_fct_accum(theirs, f0, o0)
    assert all(np.array_equal(mine[k], theirs[k]) and mine[k].dtype == theirs[k].dtype for k in restated.CAT_KEYS)
    cat.det_cat_fct_accum(theirs, f1, o1)  # an object the reference made and filled takes a pair from this side
    ref_cat.det_cat_fct_accum(mine, f1, o1)
    assert all(np.array_equal(mine[k], theirs[k]) for k in restated.CAT_KEYS)
    both = [ref_cat.det_cat_fct_merge(dict(mine), theirs), cat.det_cat_fct_merge(dict(theirs), mine)]
    for key, value in ref_cat.det_cat_fct_compute(both[0]).items():
        assert cat.det_cat_fct_compute(both[1])[key] == value
    for cond, _ in CONDS:
        mine = cont.det_cont_fct_init(conditioning=cond, thr=0.5)
        theirs = ref_cont.det_cont_fct_init(conditioning=cond, thr=0.5)
        assert list(mine) == list(theirs) and mine == theirs
        cont.det_cont_fct_accum(mine, f0, o0)
        ref_cont.det_cont_fct_accum(theirs, f0, o0)
        assert all(mine[k].dtype == theirs[k].dtype and mine[k].shape == theirs[k].shape for k in restated.MOMENTS + ["n"])
        within(as_array(mine), as_array(theirs), bar)
        cont.det_cont_fct_accum(theirs, f1, o1)
        ref_cont.det_cont_fct_accum(mine, f1, o1)
        within(as_array(mine), as_array(theirs), bar)
        copies = [{k: np.copy(v) if isinstance(v, np.ndarray) else v for k, v in obj.items()} for obj in (mine, theirs)]
        a, b = ref_cont.det_cont_fct_merge(mine, theirs), cont.det_cont_fct_merge(copies[1], copies[0])
        within(as_array(a), as_array(b), bar)
        within(scores_array(ref_cont.det_cont_fct_compute(b), restated.CONT_SCORES),
               scores_array(cont.det_cont_fct_compute(a), restated.CONT_SCORES), bar)


def test_threshold_type_decides_as_in_numpy(host_kernel):
    """On float32 fields a Python float is compared as float32 and a numpy.float64 as float64: float32(0.1) > 0.1 is
    false for the first and true for the second, as in NumPy."""
    cat, cont, _ = host_kernel
    f = np.full((3, 4), np.float32(0.1))
    o = np.full((3, 4), 1.0, np.float32)
    assert cat.det_cat_table(f, o, [0.1], return_counts=True)[1].tolist() == [[0, 12, 0, 0]]
    assert cat.det_cat_table(f, o, [np.float64(0.1)], return_counts=True)[1].tolist() == [[12, 0, 0, 0]]
    assert cat.det_cat_table(f.astype(np.float64), o, [0.1], return_counts=True)[1].tolist() == [[12, 0, 0, 0]]
    assert list(restated.counts(f, o, 0.1)) == [0, 12, 0, 0] and list(restated.counts(f, o, np.float64(0.1))) == [12, 0, 0, 0]
    o[:] = 0.05
    _, err = cont.det_cont_table(f, o, "single", 0.1, return_object=True)
    assert err["n"] == 0
    _, err = cont.det_cont_table(f, o, "single", np.float64(0.1), return_object=True)
    assert err["n"] == 12


def test_declined_inputs_go_to_the_reference_with_a_warning(golden, host_kernel, ref_pysteps):
    from pysteps.verification import detcatscores as ref_cat
    from pysteps.verification import detcontscores as ref_cont

    cat, cont, _ = host_kernel
    f, o = golden["members__f"].astype(np.float64), golden["members__o"].astype(np.float64)
    clean_f, clean_o = golden["clean__f"].astype(np.float64), golden["clean__o"].astype(np.float64)

    def same(got, want):
        assert list(got) == list(want)
        for key in want:
            np.testing.assert_array_equal(got[key], want[key])

    with np.errstate(all="ignore"):
        for axis in (0, -1, (0, 2), (-2, -1)):
            with pytest.warns(RuntimeWarning, match="running the reference's function"):
                got = cat.det_cat_fct(f, o, 1.0, axis=axis)
            same(got, ref_cat.det_cat_fct(f, o, 1.0, axis=axis))
            with pytest.warns(RuntimeWarning, match="running the reference's function"):
                got = cont.det_cont_fct(f, o, ["ME", "RMSE", "corr_p"], axis=axis)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                same(got, ref_cont.det_cont_fct(f, o, ["ME", "RMSE", "corr_p"], axis=axis))
        ints = (np.nan_to_num(clean_f).astype(np.int32), np.nan_to_num(clean_o).astype(np.int32))
        with pytest.warns(RuntimeWarning, match="dtype int32"):
            same(cat.det_cat_fct(ints[0], ints[1], 1), ref_cat.det_cat_fct(ints[0], ints[1], 1))
        with pytest.warns(RuntimeWarning, match="dtype int32"):
            same(cont.det_cont_fct(ints[0], ints[1], "mse"), ref_cont.det_cont_fct(ints[0], ints[1], "mse"))
        inf = clean_f.copy()
        inf[3, 4] = np.inf
        with pytest.warns(RuntimeWarning, match="an infinite value"):
            got = cont.det_cont_fct(inf, clean_o, ["MAE", "MSE"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            same(got, ref_cont.det_cont_fct(inf, clean_o, ["MAE", "MSE"]))
        same(cat.det_cat_fct(inf, clean_o, 1.0), ref_cat.det_cat_fct(inf, clean_o, 1.0))  # a comparison takes infinities
        # scores="" asks for the offline scores too: they are the reference's, the online ones stay this side's
        with pytest.warns(RuntimeWarning, match="offline scores corr_s and scatter"):
            got = cont.det_cont_fct(clean_f, clean_o)
        want = ref_cont.det_cont_fct(clean_f, clean_o)
        assert list(got) == list(want) and got["corr_s"] == want["corr_s"] and got["scatter"] == want["scatter"]
        within(scores_array(got, restated.CONT_SCORES), scores_array(want, restated.CONT_SCORES), 5.0 * float(golden["deviation_float64"]))
        with pytest.warns(RuntimeWarning, match="offline score corr_s"):
            assert list(cont.det_cont_fct(clean_f, clean_o, ["corr_s", "mae"])) == ["MAE", "corr_s"]
    with pytest.raises(NotImplementedError):
        cat.det_cat_table(ints[0], ints[1], [1])
    with pytest.raises(NotImplementedError, match="an infinite value"):
        cont.det_cont_table(inf, clean_o)
    with pytest.raises(ValueError):
        cont.det_cont_table(clean_f, clean_o[:5])


class _HostPlanes:
    """What the accumulator needs of a DeviceArray, on the host."""

    def __init__(self, a):
        self._a, self.shape, self.dtype = a, a.shape, a.dtype

    def view(self, i):
        return self._a[i]


def test_accumulator_on_host_stacks(golden, host_kernel, monkeypatch):
    """Without a loop that hands over device members the accumulator scores the host stack it receives: per lead time
    one table per threshold and one error object, pooled over the members in member order like a loop of _accum."""
    from pysteps_amd.device import DeviceArray

    cat, cont, detscores = host_kernel
    monkeypatch.setattr(DeviceArray, "from_host", classmethod(lambda cls, a, **kw: _HostPlanes(np.asarray(a))))
    f, o = golden["members__f"].astype(np.float64), golden["members__o"].astype(np.float64)
    obs = o[:2]
    leads = [f, f[::-1].copy()]
    thrs = [0.5, 1.0, 1.0e6]
    acc = detscores.DetScoresAccumulator(obs, thrs, conditioning="single", cont_thr=0.5, per_member=True)
    assert acc.accepts_device
    for members in leads:
        acc(members)
    assert acc.n_leadtimes == 2 and acc.received == [np.ndarray] * 2 and acc.member_counts.shape == (2, 3, 3, 4)
    for t, members in enumerate(leads):
        want = cont.det_cont_fct_init(conditioning="single", thr=0.5)
        for k in range(3):
            cont.det_cont_fct_accum(want, members[k], obs[t])
        np.testing.assert_array_equal(as_array(acc.cont_objects[t]), as_array(want))
        for i, thr in enumerate(thrs):
            table = cat.det_cat_fct_init(thr)
            for k in range(3):
                cat.det_cat_fct_accum(table, members[k], obs[t])
                assert list(acc.member_counts[t, k, i]) == list(restated.counts(members[k], obs[t], thr))
            assert acc.cat_objects[t][i] == table and acc.cat_objects[t][i]["hits"].dtype == np.dtype(int)
        assert acc.member_cont[t]["n"].shape == (3,)
    assert acc.cat_scores("csi")["CSI"].shape == (2, 3) and np.isnan(acc.cat_scores("csi")["CSI"][:, 2]).all()
    assert sorted(acc.cont_scores(["rmse", "corr_p"])) == ["RMSE", "corr_p"] and acc.cont_scores()["ME"].shape == (2,)
    with pytest.raises(ValueError):
        acc(leads[0])  # a third lead time without an observation


def test_get_method_resolves():
    from pysteps_amd import verification
    from pysteps_amd.verification import detcatscores, detcontscores

    assert verification.get_method("det_cat_fct") is detcatscores.det_cat_fct
    assert verification.get_method("DET_CONT_FCT") is detcontscores.det_cont_fct
    assert verification.DetScoresAccumulator.accepts_device and verification.det_cat_table is detcatscores.det_cat_table
    for name in ("acc", "bias", "csi", "f1", "fa", "far", "gss", "hk", "hss", "mcc", "pod", "sedi", "beta", "beta1", "beta2",
                 "corr_p", "corr_s", "drmse", "mae", "mse", "me", "nmse", "rmse", "rv", "scatter"):
        assert callable(verification.get_method(name))
    with pytest.raises(ValueError):
        verification.get_method("sal")


def test_get_method_aliases_score(golden, host_kernel):
    from pysteps_amd import verification

    f, o = golden["clean__f"], golden["clean__o"]
    assert list(verification.get_method("CSI")(f, o, thr=1.0)) == ["CSI"]
    assert list(verification.get_method("rmse")(f, o, conditioning="double", thr=0.5)) == ["RMSE"]


def test_registration_is_opt_in(ref_pysteps):
    from pysteps.verification import detcatscores as ref_cat
    from pysteps.verification import detcontscores as ref_cont

    from pysteps_amd import register
    from pysteps_amd._reference import lookup
    from pysteps_amd.verification import detcatscores, detcontscores

    def stock(mod, name):
        return lookup("verification." + mod.__name__.rsplit(".", 1)[1], name, getattr(mod, name))

    before = (ref_cat.det_cat_fct, ref_cat.det_cat_fct_accum, ref_cont.det_cont_fct, ref_cont.det_cont_fct_accum)

    def current():
        return (ref_cat.det_cat_fct, ref_cat.det_cat_fct_accum, ref_cont.det_cont_fct, ref_cont.det_cont_fct_accum)

    try:
        added = register.register()
        assert current() == before and not [a for a in added if a.startswith("verification")]
        assert register.register(detscores=True)[-4:] == ["verification:det_cat_fct", "verification:det_cat_fct_accum",
                                                          "verification:det_cont_fct", "verification:det_cont_fct_accum"]
        assert current() == (detcatscores.det_cat_fct, detcatscores.det_cat_fct_accum, detcontscores.det_cont_fct,
                             detcontscores.det_cont_fct_accum)
        assert (ref_cat._reference_det_cat_fct, ref_cat._reference_det_cat_fct_accum) == before[:2]
        assert stock(detcatscores, "det_cat_fct_accum") is before[1] and stock(detcontscores, "det_cont_fct") is before[2]
        assert register.patch_detscores() == []  # already in place
        register.unpatch_detscores()
        assert current() == before and not hasattr(ref_cat, "_reference_det_cat_fct")
        assert not [a for mod in (ref_cat, ref_cont) for a in vars(mod) if a.startswith("_reference_")]
        assert stock(detcatscores, "det_cat_fct") is before[0] and stock(detcontscores, "det_cont_fct_accum") is before[3]
        register.unpatch_detscores()  # harmless when nothing is patched
        assert current() == before
    finally:
        register.unpatch_detscores()
        register.unregister_fft()
