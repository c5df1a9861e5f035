"""Probabilistic verification scores on the device (``pysteps_amd.verification.probscores``, csrc/probscores.hip).

Counts (``n``, ``Y_sum``, ``num_idx``, ``sample_size``, the four ROC tables) are held to the integer restatement of
tests/helpers/probscores.py and to the goldens of the unmodified reference with no tolerance.  ``CRPS_sum`` is held to
``math.fsum`` over the float64 terms within ``4 * 2**-53 * sum(|term|)`` - one rounding each for the quotient, the
square and the product of a term and one at the end; the double-double accumulation is below that - and ``X_sum``
within ``2 * 2**-53 * sum(|P_f|)``.  Against the reference's goldens CRPS, reldiag ``(r, f)`` and ROC ``(POFD, POD,
area)`` are held within 5 x the reference's own deviation from the restated rule (``deviation_float32`` 1.2e-07: it
subtracts float32 members and adds float32 probabilities in float32; ``deviation_float64`` 3.8e-16), NaN positions equal.
Every case runs with NumPy input and with ``DeviceArray`` input.
"""

import warnings

import numpy as np
import pytest

from helpers import probscores as restated
from test_probscores_cpu import (BINS, DTYPES, PATH, crps_case_names, prob_case_names, reldiag_array, roc_array, typed, within)

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
_helper_cache = {}


@pytest.fixture(scope="module")
def golden():
    return np.load(PATH)


def on_device(*arrays):
    from pysteps_amd.device import DeviceArray

    return tuple(DeviceArray.from_host(np.ascontiguousarray(a)) for a in arrays)


def both_ways(*arrays):
    """The arguments as NumPy arrays, then as DeviceArrays."""
    return [("numpy", arrays), ("device", on_device(*arrays))]


def crps_terms(key, members, obs):
    """The helper's (n, sum, magnitude), computed once per case."""
    if key not in _helper_cache:
        _helper_cache[key] = restated.crps_terms(members, obs)
    return _helper_cache[key]


def check_crps_object(obj, want, label):
    n, total, magnitude = want
    assert isinstance(obj["n"], float) and obj["n"] == n, label
    err = abs(float(obj["CRPS_sum"]) - total)
    assert err <= 4.0 * EPS * magnitude, (label, float(obj["CRPS_sum"]), total)
    return err / magnitude if magnitude else 0.0


def check_bins(rdiag, roc, counted, label, min_count=10):
    """One-call objects against the helper's counting: integers exactly, X_sum to the fsum bar."""
    n_bins = len(counted["count"])
    keep = [c >= min_count for c in counted["count"]]
    assert rdiag["num_idx"].tolist() == [c if k else 0 for c, k in zip(counted["count"], keep)], label
    assert rdiag["sample_size"].tolist() == rdiag["num_idx"].tolist(), label
    assert rdiag["Y_sum"].tolist() == [e if k else 0 for e, k in zip(counted["events"], keep)], label
    worst = 0.0
    for b in range(n_bins):
        want, mag = (counted["sum"][b], counted["magnitude"][b]) if keep[b] else (0.0, 0.0)
        err = abs(float(rdiag["X_sum"][b]) - want)
        assert err <= 2.0 * EPS * mag, (label, b, float(rdiag["X_sum"][b]), want)
        worst = max(worst, err / mag if mag else 0.0)
    if roc is not None:
        assert roc_array(roc).T.tolist() == counted["roc"], label
    return worst


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", crps_case_names())
def test_crps_goldens(golden, name, dtype):
    """Ties, masks, K = 1 .. 64 on the 9-pixel and 5 x 7 planes of the golden file, and the 33 x 65 rain field."""
    from pysteps_amd.verification import probscores as ps

    bar = 5.0 * float(golden["deviation_" + dtype])
    f, o = golden[name + "__f"].astype(dtype), golden[name + "__o"].astype(dtype)
    want = golden["%s__%s__crps" % (name, dtype)]
    helper = crps_terms((name, dtype), f, o)
    sums = []
    for label, (X_f, X_o) in both_ways(f, o):
        obj = ps.CRPS_init()
        ps.CRPS_accum(obj, X_f, X_o)
        fsum_err = check_crps_object(obj, helper, (name, dtype, label))
        assert obj["n"] == want[1] and isinstance(obj["CRPS_sum"], np.float64)
        worst = within(obj["CRPS_sum"], want[0], bar)
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            worst = max(worst, within(ps.CRPS_compute(obj), want[2], bar), within(ps.CRPS(X_f, X_o), want[2], bar))
        sums.append(float(obj["CRPS_sum"]))
    assert sums[0] == sums[1] and np.array_equal(f, golden[name + "__f"].astype(dtype), equal_nan=True)  # input untouched
    print("%s %s: CRPS within %.3g of the golden (bar %.3g), %.3g x sum|term| of the helper (bar %.3g)"
          % (name, dtype, worst, bar, fsum_err, 4.0 * EPS))


def test_all_masked_plane_gives_the_references_nan(golden):
    from pysteps_amd.verification import probscores as ps

    f = golden["masked__f"].astype(np.float64)
    for fill in (np.nan, np.inf, -np.inf):
        for _, (X_f, X_o) in both_ways(f, np.full(f.shape[1:], fill)):
            obj = ps.CRPS_init()
            ps.CRPS_accum(obj, X_f, X_o)
            assert obj["n"] == 0 and obj["CRPS_sum"] == 0.0
            with pytest.warns(RuntimeWarning):
                assert np.isnan(ps.CRPS_compute(obj))
    assert np.isnan(golden["masked__float64__crps"][2])


# every K on the plane that is no multiple of the wave, every plane for a K below and one above a power of two, several
# workgroups and the second reduction stage (257 x 129 = 33153 pixels = 519 workgroups) for the largest K
SHAPES = [(K, (33, 65), ("float32", "float64")[i % 2]) for i, K in enumerate(restated.MEMBER_COUNTS)] + [
    (7, (1, 1), "float64"), (48, (1, 1), "float32"), (7, (5, 7), "float32"), (48, (5, 7), "float64"),
    (7, (257, 129), "float64"), (48, (257, 129), "float32"), (64, (257, 129), "float32"), (20, (257, 129), "float64")]


@pytest.mark.parametrize("K,shape,dtype", SHAPES)
def test_crps_shapes_against_the_helper(K, shape, dtype):
    from pysteps_amd.verification import probscores as ps

    m, n = shape
    worst = 0.0
    for ties in (True, False):
        f, o = restated.ensemble(K, m, n, 500 + K, dtype, ties=ties, bad=True)
        helper = restated.crps_terms(f, o)
        sums = []
        for label, (X_f, X_o) in both_ways(f, o):
            obj = ps.CRPS_init()
            ps.CRPS_accum(obj, X_f, X_o)
            worst = max(worst, check_crps_object(obj, helper, (K, shape, dtype, ties, label)))
            sums.append(float(obj["CRPS_sum"]))
        assert sums[0] == sums[1]
    other = np.float64 if dtype == "float32" else np.float32  # members and observation of different dtypes
    obj = ps.CRPS_init()
    ps.CRPS_accum(obj, f, o.astype(other))
    worst = max(worst, check_crps_object(obj, restated.crps_terms(f, o.astype(other)), (K, shape, dtype, "mixed")))
    print("K=%d %s %s: CRPS_sum within %.3g x sum|term| of the helper (bar %.3g)" % (K, shape, dtype, worst, 4.0 * EPS))


def test_crps_is_bit_identical_between_runs_and_positions():
    from pysteps_amd.verification import probscores as ps

    for K, (m, n), dtype in ((20, (33, 65), np.float32), (7, (257, 129), np.float64)):
        f, o = restated.ensemble(K, m, n, 600, dtype, ties=True, bad=True)
        stack = np.stack([restated.quantised((m, n), 610 + t, dtype) for t in range(5)])
        stack[3] = o
        dev_f, dev_o, dev_stack = on_device(f, o, stack)
        alone = [ps.crps_table(dev_f, dev_o, return_object=True)[1] for _ in range(2)]
        assert alone[0]["CRPS_sum"].tobytes() == alone[1]["CRPS_sum"].tobytes() and alone[0]["n"] == alone[1]["n"]
        table, obj = ps.crps_table(dev_f, dev_stack, return_object=True)
        assert table.shape == (5,) and obj["CRPS_sum"][3].tobytes() == alone[0]["CRPS_sum"].tobytes() and obj["n"][3] == alone[0]["n"]
        _, host = ps.crps_table(f, stack, return_object=True)
        assert host["CRPS_sum"].tobytes() == obj["CRPS_sum"].tobytes()
        single = ps.CRPS_init()
        ps.CRPS_accum(single, dev_f, dev_o)
        assert np.float64(single["CRPS_sum"]).tobytes() == alone[0]["CRPS_sum"].tobytes() and table[3] == ps.CRPS_compute(single)
        # several stacks per call: stack t against plane t
        stacks = np.stack([np.roll(f, t, axis=0) if t != 3 else f for t in range(5)])
        _, many = ps.crps_table(stacks, stack, return_object=True)
        assert many["CRPS_sum"][3].tobytes() == alone[0]["CRPS_sum"].tobytes()
        assert many["CRPS_sum"].tobytes() == obj["CRPS_sum"].tobytes()  # the order of the members does not matter


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", prob_case_names())
def test_binning_goldens(golden, name, dtype):
    """Probabilities j/7 with masks, the bin edges themselves with their neighbours, 0.0 and 1.0, for 10 and 7 bins."""
    from pysteps_amd.verification import probscores as ps

    bar = 5.0 * float(golden["deviation_" + dtype])
    x_min = float(golden["x_min"])
    p, o = typed(golden, name, dtype)
    worst = fsum_worst = 0.0
    for label, (P_f, X_o) in both_ways(p, o):
        roc = ps.ROC_curve_init(x_min)
        ps.ROC_curve_accum(roc, P_f, X_o)
        assert np.array_equal(roc_array(roc), golden["%s__%s__roc" % (name, dtype)]) and roc["hits"].dtype == np.dtype(int)
        with np.errstate(all="ignore"):
            pofd, pod, area = ps.ROC_curve(P_f, X_o, x_min, compute_area=True)
        worst = max(worst, within(np.array([pofd, pod]), golden["%s__%s__curve" % (name, dtype)], bar),
                    within(area, golden["%s__%s__area" % (name, dtype)], bar))
        for n_bins in BINS:
            tag = "%s__%s__b%d" % (name, dtype, n_bins)
            rdiag = ps.reldiag_init(x_min, n_bins)
            ps.reldiag_accum(rdiag, P_f, X_o)
            assert np.array_equal(reldiag_array(rdiag)[1:], golden[tag + "__reldiag"][1:]), (tag, label)
            assert all(rdiag[k].dtype == np.dtype(int) for k in restated.BIN_KEYS[1:])
            counted = restated.bin_counts(p, o, x_min, edges=rdiag["bin_edges"], prob_thrs=roc["prob_thrs"])
            fsum_worst = max(fsum_worst, check_bins(rdiag, roc, counted, (tag, label)))
            with np.errstate(all="ignore"):
                worst = max(worst, within(rdiag["X_sum"], golden[tag + "__reldiag"][0], bar),
                            within(np.stack(ps.reldiag_compute(rdiag)), golden[tag + "__rf"], bar),
                            within(np.stack(ps.reldiag(P_f, X_o, x_min, n_bins=n_bins)), golden[tag + "__rf"], bar))
    assert np.array_equal(p, golden[name + "__p"].astype(dtype), equal_nan=True)  # the input is not modified
    print("%s %s: reldiag and ROC within %.3g of the golden (bar %.3g), X_sum %.3g x sum|P_f| of the helper (bar %.3g)"
          % (name, dtype, worst, bar, fsum_worst, 2.0 * EPS))


@pytest.mark.parametrize("dtype", DTYPES)
def test_min_count_applies_to_each_call(golden, dtype):
    """A call whose bin has 9 samples adds zeros, one whose bin has 10 adds its sums: the golden's two-call objects."""
    from pysteps_amd.verification import probscores as ps

    bar = 5.0 * float(golden["deviation_" + dtype])
    x_min = float(golden["x_min"])
    for resident in (False, True):
        for n_bins in BINS:
            rdiag, roc = ps.reldiag_init(x_min, n_bins), ps.ROC_curve_init(x_min)
            for i, name in enumerate(("mincount_a", "mincount_b")):
                args = typed(golden, name, dtype)
                args = on_device(*args) if resident else args
                ps.reldiag_accum(rdiag, *args)
                ps.ROC_curve_accum(roc, *args)
                if n_bins == 10:
                    assert rdiag["num_idx"][:3].tolist() == ([0, 10, 30], [10, 10, 30])[i] and (i or rdiag["X_sum"][0] == 0.0)
            want = golden["mincount_ab__%s__b%d__reldiag" % (dtype, n_bins)]
            assert np.array_equal(reldiag_array(rdiag)[1:], want[1:])
            within(rdiag["X_sum"], want[0], bar)
            with np.errstate(all="ignore"):
                within(np.stack(ps.reldiag_compute(rdiag)), golden["mincount_ab__%s__b%d__rf" % (dtype, n_bins)], bar)
                pofd, pod, area = ps.ROC_curve_compute(roc, True)
            assert np.array_equal(roc_array(roc), golden["mincount_ab__%s__roc" % dtype])
            within(np.array([pofd, pod]), golden["mincount_ab__%s__curve" % dtype], bar)
            within(area, golden["mincount_ab__%s__area" % dtype], bar)


@pytest.mark.parametrize("shape,K,n_bins,n_thrs,p_dtype,o_dtype", [
    ((1, 1), 7, 10, 10, "float64", "float32"), ((5, 7), 3, 7, 10, "float32", "float32"), ((33, 65), 48, 10, 10, "float64", "float64"),
    ((33, 65), 20, 64, 64, "float32", "float64"), ((257, 129), 7, 7, 12, "float64", "float32"), ((257, 129), 64, 10, 10, "float32", "float32")])
def test_binning_shapes_against_the_helper(shape, K, n_bins, n_thrs, p_dtype, o_dtype):
    """One pixel, planes that are no multiple of the wave, several workgroups (257 x 129: 519), the most bins and
    thresholds one pass takes, probabilities and observations of different dtypes, NaN and +-inf on either side."""
    from pysteps_amd.verification import probscores as ps

    p = restated.probabilities(K, shape, 700 + K, p_dtype)
    o = restated.rainy(shape, 701 + K, o_dtype)
    if p.size >= 7:
        for pixel, value in enumerate((np.nan, np.inf, -np.inf)):
            p.reshape(-1)[pixel] = value
            o.reshape(-1)[3 + pixel] = value
    x_min = 0.5
    worst = 0.0
    for min_count in (10, 1):
        first = None
        for label, (P_f, X_o) in both_ways(p, o):
            rdiag, roc = ps.reldiag_init(x_min, n_bins, min_count), ps.ROC_curve_init(x_min, n_thrs)
            ps.reldiag_accum(rdiag, P_f, X_o)
            ps.ROC_curve_accum(roc, P_f, X_o)
            if first is None:
                counted = restated.bin_counts(p, o, x_min, edges=rdiag["bin_edges"], prob_thrs=roc["prob_thrs"])
                first = (rdiag, roc)
            worst = max(worst, check_bins(rdiag, roc, counted, (shape, K, n_bins, label), min_count))
            pair = (ps.reldiag_init(x_min, n_bins, min_count), ps.ROC_curve_init(x_min, n_thrs))
            ps._accum_both(pair[0], pair[1], P_f, X_o)  # one read for both objects: the same bits
            assert reldiag_array(pair[0]).tobytes() == reldiag_array(rdiag).tobytes() and np.array_equal(roc_array(pair[1]), roc_array(roc))
            assert reldiag_array(first[0]).tobytes() == reldiag_array(rdiag).tobytes()
    print("%s K=%d %d bins: X_sum within %.3g x sum|P_f| of the helper (bar %.3g)" % (shape, K, n_bins, worst, 2.0 * EPS))


def test_two_accum_calls_on_halves_equal_the_helpers_two_calls():
    from pysteps_amd.verification import probscores as ps

    K, (m, n) = 7, (33, 65)
    f, o = restated.ensemble(K, m, n, 800, np.float32, ties=False, bad=True)
    p = restated.probabilities(K, (m, n), 801)
    halves = [(slice(0, 17), ), (slice(17, m), )]
    crps = ps.CRPS_init()
    rdiag, roc = ps.reldiag_init(0.5, 7), ps.ROC_curve_init(0.5)
    total, n_want, terms, mags, tables, bits = None, 0, [], 0.0, np.zeros((10, 4), int), []
    for rows in halves:
        f_half, o_half, p_half = np.ascontiguousarray(f[:, rows[0]]), np.ascontiguousarray(o[rows[0]]), np.ascontiguousarray(p[rows[0]])
        ps.CRPS_accum(crps, *on_device(f_half, o_half))
        ps.reldiag_accum(rdiag, p_half, o_half)
        ps.ROC_curve_accum(roc, *on_device(p_half, o_half))
        n_half, s_half, mag_half = restated.crps_terms(f_half, o_half)
        n_want, mags = n_want + n_half, mags + mag_half
        terms.append(s_half)
        counted = restated.bin_counts(p_half, o_half, 0.5, edges=rdiag["bin_edges"], prob_thrs=roc["prob_thrs"])
        total = restated.add_to_reldiag(total, counted, 10)
        tables += np.array(counted["roc"])
        bits.append(float(crps["CRPS_sum"]))
    assert crps["n"] == n_want and abs(float(crps["CRPS_sum"]) - (terms[0] + terms[1])) <= 4.0 * EPS * mags
    assert [rdiag[k].tolist() for k in restated.BIN_KEYS[1:]] == [total[k] for k in restated.BIN_KEYS[1:]]
    for b, parts in enumerate(total["X_sum"]):
        assert abs(float(rdiag["X_sum"][b]) - sum(parts)) <= 2.0 * EPS * total["X_mag"][b]
    assert np.array_equal(roc_array(roc).T, tables)


def test_accumulator_equals_excprob_and_the_accum_functions_by_hand():
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.postprocessing import ensemblestats
    from pysteps_amd.verification import ProbScoresAccumulator
    from pysteps_amd.verification import probscores as ps

    leads = [restated.ensemble(7, 33, 65, 900 + t, np.float32, ties=bool(t % 2), bad=True) for t in range(3)]
    members = np.stack([lead[0] for lead in leads])
    obs = np.stack([lead[1] for lead in leads]).astype(np.float64)
    thrs = [0.5, 2.0]
    objects = []
    for resident in (True, False):
        acc = ProbScoresAccumulator(DeviceArray.from_host(obs) if resident else obs, thrs, n_bins=7, n_prob_thrs=12, min_count=5)
        assert acc.accepts_device
        for t in range(3):
            acc(DeviceArray.from_host(members[t]) if resident else members[t])
        assert acc.received == [DeviceArray if resident else np.ndarray] * 3 and acc.n_leadtimes == 3
        with pytest.raises(ValueError):
            acc(members[0])  # a fourth lead time without an observation
        for t in range(3):
            want = ps.CRPS_init()
            ps.CRPS_accum(want, members[t], obs[t])
            assert acc.crps_objects[t] == want
            probs = ensemblestats.excprob(members[t], thrs)
            for i, thr in enumerate(thrs):
                rdiag, roc = ps.reldiag_init(thr, 7, 5), ps.ROC_curve_init(thr, 12)
                ps.reldiag_accum(rdiag, probs[i], obs[t])
                ps.ROC_curve_accum(roc, probs[i], obs[t])
                assert reldiag_array(acc.reldiag_objects[t][i]).tobytes() == reldiag_array(rdiag).tobytes()
                assert np.array_equal(roc_array(acc.roc_objects[t][i]), roc_array(roc)) and acc.roc_objects[t][i]["X_min"] == thr
                counted = restated.bin_counts(probs[i], obs[t], thr, edges=rdiag["bin_edges"], prob_thrs=roc["prob_thrs"])
                check_bins(rdiag, roc, counted, (t, i), 5)
                with np.errstate(all="ignore"):
                    assert np.array_equal(np.stack(acc.reldiag(t, i)), np.stack(ps.reldiag_compute(rdiag)), equal_nan=True)
                    got, want_roc = acc.roc(t, i, True), ps.ROC_curve_compute(roc, True)
                    assert np.array_equal(np.array(got[:2]), np.array(want_roc[:2]), equal_nan=True) and len(acc.roc(t, i)) == 2
                    assert np.array_equal(got[2], want_roc[2], equal_nan=True)
        crps = acc.crps()
        assert crps.shape == (3,) and crps.dtype == np.float64 and np.isfinite(crps).all() and (crps > 0).all()
        objects.append((crps, [[reldiag_array(o) for o in row] for row in acc.reldiag_objects], [[roc_array(o) for o in row] for row in acc.roc_objects]))
    assert objects[0][0].tobytes() == objects[1][0].tobytes()  # resident and host members give equal objects
    assert np.array(objects[0][1]).tobytes() == np.array(objects[1][1]).tobytes() and np.array_equal(objects[0][2], objects[1][2])
    only_crps = ProbScoresAccumulator(obs, [], crps=True)
    only_crps(members[0])
    assert only_crps.crps().tobytes() == objects[0][0][:1].tobytes() and only_crps.reldiag_objects == [[]]
    with pytest.raises(ValueError):
        ProbScoresAccumulator(obs, [], crps=False)


def test_registered_reference_functions_run_on_the_device(golden, ref_pysteps):
    from pysteps.verification import probscores as ref

    from pysteps_amd import register
    from pysteps_amd.verification import probscores as ps

    x_min = float(golden["x_min"])
    f, o = golden["rain_7__f"].astype(np.float64), golden["rain_7__o"].astype(np.float64)
    p, po = typed(golden, "k7", "float64")
    bar = 5.0 * float(golden["deviation_float64"])
    many, obs = restated.ensemble(65, 3, 4, 7, np.float64)
    with np.errstate(all="ignore"):
        want = (ref.CRPS(f, o), ref.reldiag(p, po, x_min), ref.ROC_curve(p, po, x_min, compute_area=True), ref.CRPS(many, obs))
    try:
        assert "verification:CRPS_accum" in register.register(probscores=True)
        assert ref.CRPS is ps.CRPS and ref.reldiag_accum is ps.reldiag_accum
        with np.errstate(all="ignore"):
            with warnings.catch_warnings():  # served: no warning
                warnings.simplefilter("error", RuntimeWarning)
                within(ref.CRPS(f, o), want[0], bar)
                got = ref.ROC_curve(p, po, x_min, compute_area=True)
            within(np.stack(ref.reldiag(p, po, x_min)), np.stack(want[1]), bar)
            assert got == want[2]
            with pytest.warns(RuntimeWarning, match="65 members"):
                assert ref.CRPS(many, obs) == want[3]
    finally:
        register.unpatch_probscores()
        register.unregister_fft()
    assert ref.CRPS is not ps.CRPS


def test_entry_points_refuse_with_an_error_code():
    from pysteps_amd import _lib
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.verification import probscores as ps

    f = DeviceArray.from_host(np.zeros((3, 8, 9), np.float32))
    o = DeviceArray.from_host(np.zeros((8, 9), np.float32))
    with pytest.raises(ValueError):
        ps._crps_sums(f, o, 1, 65, 1, True)  # more members than a thread sorts
    with pytest.raises(ValueError):
        ps._crps_sums(f, o, 1, 3, 0, True)  # no pixel
    with pytest.raises(ValueError):
        ps._bins(o, o, 72, 0.5, np.linspace(0.0, 1.0, 67), None)  # 66 bins
    with pytest.raises(ValueError):
        ps._bins(o, o, 72, 0.5, None, np.linspace(0.0, 1.0, 65))  # 65 thresholds
    with pytest.raises(ValueError):
        ps._bins(o, o, 72, 0.5, None, None)  # nothing to count
    weights = ps.crps_weights(3)
    counts, sums = DeviceArray((1,), np.uint64), DeviceArray((1, 2), np.float64)
    lib = _lib.lib()
    assert lib.psh_crps_sums_dev(f.ptr + 2, 0, 1, o.ptr, 0, 1, 3, 72, weights.ctypes.data, counts.ptr, sums.ptr) != 0
    assert lib.psh_crps_sums_dev(None, 0, 1, o.ptr, 0, 1, 3, 72, weights.ctypes.data, counts.ptr, sums.ptr) != 0
    assert lib.psh_crps_sums_dev(f.ptr, 0, 1, o.ptr, 0, 1, 3, 72, weights.ctypes.data, counts.ptr, sums.ptr) == 0
    assert counts.to_host().tolist() == [72] and sums.to_host().tolist() == [[0.0, 0.0]]
    with pytest.raises(NotImplementedError):
        ps.crps_table(DeviceArray.from_host(np.zeros((65, 2, 2), np.float32)), DeviceArray.from_host(np.zeros((2, 2), np.float32)))
    with pytest.raises(NotImplementedError):  # resident fields cannot go to the reference
        ps.reldiag_accum(ps.reldiag_init(0.5, 65), o, o)
