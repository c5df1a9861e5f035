"""Deterministic verification scores on the device (``pysteps_amd.verification.detcatscores`` / ``detcontscores``,
csrc/detscores.hip).

Contingency counts are held to the integer restatement of tests/helpers/detscores.py and to the goldens of the
unmodified reference with no tolerance, categorical scores bit for bit.  The raw sums are held to ``math.fsum`` over the
float64 terms within ``4 * 2**-53 * sum(|term|)``: one rounding per term and one at the end.  Continuous moments and
scores are held to the reference's within 5 x the reference's own deviation from the definitions (9.73e-07 relative for
float32 fields, 6.8e-15 for float64 fields: tests/test_detscores_cpu.py), NaN positions equal.
"""

import os
import warnings

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import detscores as restated
from test_detscores_cpu import CONDS, DTYPES, as_array, case_names, scores_array, thresholds_of, within

pytestmark = pytest.mark.gpu

PATH = os.path.join(GOLDEN, "detscores_reference.npz")
EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def golden():
    return np.load(PATH)


def check_raw(pred, obs, counts, sums, conditioning=None, thr=0.0):
    """One forecast's device counts (4,) and sums (11, 2) against the helper."""
    want_counts, want, mags = restated.raw_sums(pred, obs, conditioning, thr)
    assert [int(c) for c in counts[:3]] == list(want_counts) and int(counts[3]) == 0
    for i, name in enumerate(restated.SUMS):
        got = float(sums[i, 0] + sums[i, 1])
        assert abs(got - want[name]) <= 4.0 * EPS * mags[name], (name, got, want[name])


def raw(pred, obs, shared=False, conditioning=0, thr_f=0.0, thr_o=0.0):
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.verification import detcontscores

    K = pred.shape[0] if pred.ndim == 3 else 1
    dev_f = pred if isinstance(pred, DeviceArray) else DeviceArray.from_host(np.ascontiguousarray(pred))
    dev_o = obs if isinstance(obs, DeviceArray) else DeviceArray.from_host(np.ascontiguousarray(obs))
    return detcontscores._sums(dev_f, dev_o, K, int(np.prod(pred.shape[-2:])), shared, conditioning, thr_f, thr_o)


@pytest.mark.parametrize("resident", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", case_names())
def test_goldens(golden, name, dtype, resident):
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.verification import detcatscores as cat
    from pysteps_amd.verification import detcontscores as cont

    bar = 5.0 * float(golden["deviation_" + dtype])
    f, o = golden[name + "__f"].astype(dtype), golden[name + "__o"].astype(dtype)
    args = (DeviceArray.from_host(f), DeviceArray.from_host(o)) if resident else (f, o)
    axis = (1, 2) if f.ndim == 3 else None
    thrs = thresholds_of(golden)
    for i, thr in enumerate(thrs):
        obj = cat.det_cat_fct_init(thr, axis)
        cat.det_cat_fct_accum(obj, *args)
        assert all(obj[k].dtype == np.dtype(int) for k in restated.CAT_KEYS)
        np.testing.assert_array_equal(np.stack([obj[k] for k in restated.CAT_KEYS]), golden["%s__%s__counts" % (name, dtype)][i])
        with np.errstate(all="ignore"):
            np.testing.assert_array_equal(scores_array(cat.det_cat_fct(args[0], args[1], thr, axis=axis), restated.CAT_SCORES),
                                          golden["%s__%s__cat" % (name, dtype)][i])
    with np.errstate(all="ignore"):
        table = cat.det_cat_table(args[0], args[1], thrs)
    np.testing.assert_array_equal(scores_array(table, restated.CAT_SCORES), np.moveaxis(golden["%s__%s__cat" % (name, dtype)], 0, -1))
    worst = 0.0
    for cond, tag in CONDS:
        key = "%s__%s__%s" % (name, dtype, tag)
        obj = cont.det_cont_fct_init(axis=axis, conditioning=cond, thr=restated.CONT_THR)
        cont.det_cont_fct_accum(obj, *args)
        worst = max(worst, within(as_array(obj), golden[key + "__obj"], bar))
        with np.errstate(all="ignore"):
            online = cont.det_cont_fct(args[0], args[1], restated.CONT_SCORES, axis=axis, conditioning=cond, thr=restated.CONT_THR)
        worst = max(worst, within(scores_array(online, restated.CONT_SCORES), golden[key + "__cont"], bar))
    print("%s %s: moments and continuous scores within %.3g of the golden (bar %.3g)" % (name, dtype, worst, bar))
    if not resident:
        assert np.array_equal(f, golden[name + "__f"].astype(dtype), equal_nan=True)  # the input is not modified


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_accumulations_and_a_merge(golden, dtype):
    from pysteps_amd.verification import detcatscores as cat
    from pysteps_amd.verification import detcontscores as cont

    bar = 5.0 * float(golden["deviation_" + dtype])
    pairs = [(golden["merge__f%d" % i].astype(dtype), golden["merge__o%d" % i].astype(dtype)) for i in range(3)]
    a, b = cat.det_cat_fct_init(1.0), cat.det_cat_fct_init(1.0)
    cat.det_cat_fct_accum(a, *pairs[0])
    cat.det_cat_fct_accum(a, *pairs[1])
    cat.det_cat_fct_accum(b, *pairs[2])
    merged = cat.det_cat_fct_merge(a, b)
    np.testing.assert_array_equal(np.stack([merged[k] for k in restated.CAT_KEYS]), golden["merge__%s__cat_merged" % dtype])
    np.testing.assert_array_equal(scores_array(cat.det_cat_fct_compute(merged), restated.CAT_SCORES), golden["merge__%s__cat" % dtype])
    for cond, tag in CONDS:
        key = "merge__%s__%s" % (dtype, tag)
        a = cont.det_cont_fct_init(conditioning=cond, thr=restated.CONT_THR)
        b = cont.det_cont_fct_init(conditioning=cond, thr=restated.CONT_THR)
        cont.det_cont_fct_accum(a, *pairs[0])
        cont.det_cont_fct_accum(a, *pairs[1])
        cont.det_cont_fct_accum(b, *pairs[2])
        within(as_array(a), golden[key + "__a"], bar)
        merged = cont.det_cont_fct_merge(a, b)
        within(as_array(merged), golden[key + "__merged"], bar)
        within(scores_array(cont.det_cont_fct_compute(merged), restated.CONT_SCORES), golden[key + "__cont"], bar)


@pytest.mark.parametrize("shape,dtype,K", [((1, 1), "float32", 1), ((1, 1), "float64", 2), ((33, 47), "float32", 3),
                                           ((33, 47), "float64", 3), ((61, 130), "float64", 2)])
def test_small_shapes_against_the_helper(shape, dtype, K):
    """Raw sums and counts: misaligned member bases (33 * 47 % 4 = 3), a stack against a shared observation and against
    a stack, forecast and observation of different dtypes, all three conditionings."""
    from pysteps_amd.verification import detcatscores as cat

    m, n = shape
    pairs = [restated.pair(m, n, 40 + k, dtype, nan_f=0.02 * (m > 1), nan_o=0.03 * (m > 1)) for k in range(K)]
    fct, obs = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    other = np.float64 if dtype == "float32" else np.float32
    for conditioning, code in ((None, 0), ("single", 1), ("double", 2)):
        if m == 1 and code:
            continue
        counts, sums = raw(fct, obs, False, code, 0.5, 0.5)
        shared_counts, shared_sums = raw(fct, obs[0], True, code, 0.5, 0.5)
        mixed_counts, mixed_sums = raw(fct, obs.astype(other), False, code, 0.5, 0.5)
        for k in range(K):
            check_raw(fct[k], obs[k], counts[k], sums[k], conditioning, 0.5)
            check_raw(fct[k], obs[0], shared_counts[k], shared_sums[k], conditioning, 0.5)
            check_raw(fct[k], obs[k].astype(other), mixed_counts[k], mixed_sums[k], conditioning, 0.5)
    thrs = [0.25 * j for j in range(17)]  # 9 and 17 thresholds cross the block of 8 per pass
    for count in (9, 17):
        _, table = cat.det_cat_table(fct, obs, thrs[:count], return_counts=True)
        _, shared = cat.det_cat_table(fct, obs[0], thrs[:count], return_counts=True)
        _, mixed = cat.det_cat_table(fct, obs.astype(other), thrs[:count], return_counts=True)
        assert table.shape == (K, count, 4)
        for k in range(K):
            for i in (0, 7, 8, count - 1):
                assert [int(c) for c in table[k, i]] == list(restated.counts(fct[k], obs[k], thrs[i]))
                assert [int(c) for c in shared[k, i]] == list(restated.counts(fct[k], obs[0], thrs[i]))
                assert [int(c) for c in mixed[k, i]] == list(restated.counts(fct[k], obs[k].astype(other), thrs[i]))


def test_all_nan_field_leaves_the_object_untouched():
    from pysteps_amd.verification import detcatscores as cat
    from pysteps_amd.verification import detcontscores as cont

    f, o = restated.pair(33, 47, 3, np.float64)
    err = cont.det_cont_fct_init()
    cont.det_cont_fct_accum(err, f, o)
    before = as_array(err)
    with pytest.warns(RuntimeWarning, match="Mean of empty slice"):
        cont.det_cont_fct_accum(err, np.full((33, 47), np.nan), o)
    np.testing.assert_array_equal(as_array(err), before)
    fresh = cont.det_cont_fct_init()
    with pytest.warns(RuntimeWarning):
        cont.det_cont_fct_accum(fresh, np.full((33, 47), np.nan, np.float32), o)
    assert fresh["n"] == 0 and np.all(as_array(fresh) == 0.0)
    table = cat.det_cat_fct_init(0.5)
    cat.det_cat_fct_accum(table, np.full((33, 47), np.nan), o)
    assert table["hits"] == 0 and table["false_alarms"] == 0 and table["misses"] + table["correct_negatives"] == 33 * 47


@pytest.mark.parametrize("shape,dtype,K", [((1226, 761), "float64", 3), ((4096, 4096), "float32", 2)])
def test_large_shapes_grid_stride_and_many_workgroups(shape, dtype, K):
    """Counts exactly, sums to the fsum bar; the first member against its own observation, the last against the shared one."""
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.verification import detcatscores as cat

    m, n = shape
    rng = np.random.default_rng(7)
    base = restated.field(m, n, 70, dtype, nan=0.001)
    fct = np.stack([np.roll(base, 3 * k + 1, axis=1) for k in range(K)])
    obs = (np.roll(base, (2, -1), axis=(0, 1)) * rng.uniform(0.5, 1.5, (m, n))).astype(dtype)
    dev_f, dev_o = DeviceArray.from_host(fct), DeviceArray.from_host(obs)
    counts, sums = raw(dev_f, dev_o, True, 1, 0.5, 0.5)
    _, table = cat.det_cat_table(dev_f, dev_o, [0.5, 2.0], return_counts=True)
    for k in (0, K - 1):
        if k == K - 1 or m < 4096:  # fsum over 16.7 million terms takes seconds: one member at the largest shape
            check_raw(fct[k], obs, counts[k], sums[k], "single", 0.5)
        with np.errstate(invalid="ignore"):
            for i, thr in enumerate((0.5, 2.0)):
                pb, ob = fct[k] > thr, obs > thr
                want = [int((pb & ob).sum()), int((~pb & ob).sum()), int((pb & ~ob).sum()), int((~pb & ~ob).sum())]
                assert [int(c) for c in table[k, i]] == want


def test_results_are_bit_identical_between_runs_and_splits():
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.verification import detcatscores as cat

    pairs = [restated.pair(61, 131, 80 + k, np.float32, nan_f=0.01) for k in range(6)]  # 61 * 131 % 4 = 3
    fct, obs = np.stack([p[0] for p in pairs]), pairs[0][1]
    dev_f, dev_o = DeviceArray.from_host(fct), DeviceArray.from_host(obs)
    first, again = raw(dev_f, dev_o, True, 2, 0.5, 0.5), raw(dev_f, dev_o, True, 2, 0.5, 0.5)
    assert np.array_equal(first[0], again[0]) and first[1].tobytes() == again[1].tobytes()
    halves = [raw(fct[:3], obs, True, 2, 0.5, 0.5), raw(np.ascontiguousarray(fct[3:]), obs, True, 2, 0.5, 0.5)]  # own uploads
    assert np.concatenate([h[0] for h in halves]).tobytes() == first[0].tobytes()
    assert np.concatenate([h[1] for h in halves]).tobytes() == first[1].tobytes()
    thrs = [0.1 * j for j in range(9)]
    whole = cat.det_cat_table(dev_f, dev_o, thrs, return_counts=True)[1]
    parts = [cat.det_cat_table(fct[:3], obs, thrs, return_counts=True)[1], cat.det_cat_table(fct[3:], obs, thrs, return_counts=True)[1]]
    assert np.array_equal(np.concatenate(parts), whole) and np.array_equal(whole, cat.det_cat_table(dev_f, dev_o, thrs, return_counts=True)[1])


def test_accumulator_equals_a_loop_of_accum_calls():
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.verification import DetScoresAccumulator
    from pysteps_amd.verification import detcatscores as cat
    from pysteps_amd.verification import detcontscores as cont

    pairs = [restated.pair(33, 47, 90 + k, np.float32, nan_f=0.02, nan_o=0.01) for k in range(6)]
    members32 = np.stack([p[0] for p in pairs]).reshape(2, 3, 33, 47)
    obs = np.stack([pairs[0][1], pairs[1][1]]).astype(np.float64)
    thrs = [0.5, 2.0]
    for resident in (True, False):
        acc = DetScoresAccumulator(obs, thrs, conditioning="single", cont_thr=0.5, per_member=True)
        for t in range(2):
            acc(DeviceArray.from_host(members32[t]) if resident else members32[t])
        assert acc.received == [DeviceArray if resident else np.ndarray] * 2
        block = members32.astype(np.float64) if resident else members32  # resident float32 members count as widened
        for t in range(2):
            want = cont.det_cont_fct_init(conditioning="single", thr=0.5)
            for k in range(3):
                cont.det_cont_fct_accum(want, block[t, k], obs[t])
            np.testing.assert_array_equal(as_array(acc.cont_objects[t]), as_array(want))
            for i, thr in enumerate(thrs):
                table = cat.det_cat_fct_init(thr)
                for k in range(3):
                    cat.det_cat_fct_accum(table, block[t, k], obs[t])
                assert acc.cat_objects[t][i] == table
        assert acc.cat_scores()["CSI"].shape == (2, 2) and np.isfinite(acc.cont_scores()["RMSE"]).all()


def test_accumulator_inside_a_real_steps_run(ref_pysteps):
    """The real pysteps.nowcasts.steps with the resident loop and return_output=False: the accumulator receives the
    members where they lie and no member is downloaded."""
    from pysteps import nowcasts

    from pysteps_amd import register
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.nowcasts import utils as loop
    from pysteps_amd.verification import DetScoresAccumulator
    from test_callers_gpu import _steps_inputs, _steps_kwargs

    frames, V = _steps_inputs(256, 256)
    kw = _steps_kwargs()
    n_leadtimes = 3
    observations = np.stack([np.roll(frames[-1], (2 * (t + 1), 3 * (t + 1)), axis=(0, 1)) for t in range(n_leadtimes)])
    steps = nowcasts.get_method("steps")
    try:
        register.register(patch_main_loop=True)
        acc = DetScoresAccumulator(DeviceArray.from_host(observations), [-5.0, 0.0, 5.0])  # dBR
        out = steps(frames, V, n_leadtimes, extrap_method="semilagrangian_hip", callback=acc, return_output=False, **kw)
        assert out is None and "download" not in loop.last_run_stats and "callback" in loop.last_run_stats
        assert acc.n_leadtimes == n_leadtimes and acc.received == [DeviceArray] * n_leadtimes
        pixels = kw["n_ens_members"] * 256 * 256
        for t in range(n_leadtimes):
            for table in acc.cat_objects[t]:
                assert sum(int(table[k]) for k in restated.CAT_KEYS) == pixels
            assert 0 < acc.cont_objects[t]["n"] <= pixels
        csi, rmse = acc.cat_scores("csi")["CSI"], acc.cont_scores("rmse")["RMSE"]
        assert csi.shape == (n_leadtimes, 3) and np.isfinite(csi).all() and 0.0 <= csi.min() and 0.0 < csi.max() <= 1.0
        assert rmse.shape == (n_leadtimes,) and np.isfinite(rmse).all() and rmse.min() > 0.0
    finally:
        register.unpatch_main_loop()
        register.unregister_fft()


def test_registered_reference_functions_run_on_the_device_and_decline(golden, ref_pysteps):
    from pysteps.verification import detcatscores as ref_cat
    from pysteps.verification import detcontscores as ref_cont

    from pysteps_amd import register
    from pysteps_amd.verification import detcatscores as cat
    from pysteps_amd.verification import detcontscores as cont

    f, o = golden["members__f"].astype(np.float64), golden["members__o"].astype(np.float64)
    names = ["ME", "RMSE", "corr_p"]

    def same(got, want):
        assert list(got) == list(want)
        for key in want:
            np.testing.assert_array_equal(got[key], want[key])

    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want_cat = {axis: ref_cat.det_cat_fct(f, o, 1.0, axis=axis) for axis in (None, (1, 2), 0, -1)}
        want_cont = {axis: ref_cont.det_cont_fct(f, o, names, axis=axis) for axis in (None, (1, 2), 0, -1)}
        ints = (np.nan_to_num(f).astype(np.int32), np.nan_to_num(o).astype(np.int32))
        inf = np.nan_to_num(f[0])
        inf[3, 4] = np.inf
        want_ints, want_inf = ref_cont.det_cont_fct(ints[0], ints[1], names), ref_cont.det_cont_fct(inf, np.nan_to_num(o[0]), names)
        want_all = ref_cont.det_cont_fct(np.nan_to_num(f[0]), np.nan_to_num(o[0]))
    try:
        assert "verification:det_cont_fct_accum" in register.register(detscores=True)
        assert ref_cat.det_cat_fct is cat.det_cat_fct and ref_cont.det_cont_fct_accum is cont.det_cont_fct_accum
        bar = 5.0 * float(golden["deviation_float64"])
        with np.errstate(all="ignore"):
            for axis in (None, (1, 2)):  # served: no warning
                with warnings.catch_warnings():
                    warnings.simplefilter("error", RuntimeWarning)
                    same(ref_cat.det_cat_fct(f, o, 1.0, axis=axis), want_cat[axis])
                    got = ref_cont.det_cont_fct(f, o, names, axis=axis)
                within(scores_array(got, names), scores_array(want_cont[axis], names), bar)
            for axis in (0, -1):  # declined: the reference's results with a warning
                with pytest.warns(RuntimeWarning, match="running the reference's function"):
                    same(ref_cat.det_cat_fct(f, o, 1.0, axis=axis), want_cat[axis])
                with pytest.warns(RuntimeWarning, match="running the reference's function"):
                    same(ref_cont.det_cont_fct(f, o, names, axis=axis), want_cont[axis])
            with pytest.warns(RuntimeWarning, match="dtype int32"):
                same(ref_cont.det_cont_fct(ints[0], ints[1], names), want_ints)
            with pytest.warns(RuntimeWarning, match="an infinite value"):
                same(ref_cont.det_cont_fct(inf, np.nan_to_num(o[0]), names), want_inf)
            with pytest.warns(RuntimeWarning, match="offline scores corr_s and scatter"):
                got = ref_cont.det_cont_fct(np.nan_to_num(f[0]), np.nan_to_num(o[0]))
            assert list(got) == list(want_all) and got["corr_s"] == want_all["corr_s"] and got["scatter"] == want_all["scatter"]
            within(scores_array(got, restated.CONT_SCORES), scores_array(want_all, restated.CONT_SCORES), bar)
    finally:
        register.unpatch_detscores()
        register.unregister_fft()
    assert ref_cat.det_cat_fct is not cat.det_cat_fct


def test_entry_points_refuse_with_an_error_code():
    from pysteps_amd import _lib
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.verification import detcatscores as cat
    from pysteps_amd.verification import detcontscores as cont

    f = DeviceArray.from_host(np.zeros((8, 9), np.float32))
    with pytest.raises(ValueError):
        cont._sums(f, f, 1, 72, True, 3, 0.0, 0.0)  # no such conditioning
    with pytest.raises(ValueError):
        cont._sums(f, f, 70000, 72, True, 0, 0.0, 0.0)  # more forecasts than a launch takes
    with pytest.raises(ValueError):
        cat._counts(f, f, 1, 0, True, [0.5], [0.5])  # no pixel
    out = DeviceArray((1, 1, 4), np.uint64)
    thr = np.array([0.5])
    assert _lib.lib().psh_detcat_counts_dev(f.ptr + 2, 0, f.ptr, 0, 1, 1, 8, thr.ctypes.data, thr.ctypes.data, 1, out.ptr) != 0
    assert _lib.lib().psh_detcat_counts_dev(None, 0, f.ptr, 0, 1, 1, 8, thr.ctypes.data, thr.ctypes.data, 1, out.ptr) != 0
    with pytest.raises(NotImplementedError):
        cont.det_cont_fct(f, f, "")  # resident fields cannot go to the reference for the offline scores
    with pytest.raises(NotImplementedError):
        cat.det_cat_fct(DeviceArray.from_host(np.zeros((2, 8, 9), np.float32)), DeviceArray.from_host(np.zeros((2, 8, 9), np.float32)), 0.5, axis=0)
    assert cat._counts(f, f, 1, 72, True, [-1.0, 0.0], [-1.0, 0.0]).tolist() == [[[72, 0, 0, 0], [0, 0, 0, 72]]]
