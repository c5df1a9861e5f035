"""The probabilistic verification scores' host side (no GPU): the restatement of tests/helpers/probscores.py against the
reference's goldens, the host arithmetic (``_compute``) bit for bit, and the Python layer (objects, ``get_method``,
fall-back, registration) with the restatement standing in for the two entry points.

Yardstick for ``CRPS_sum`` and ``X_sum``: the reference's own error.  tools/make_golden_probscores.py measured both
against the restated rule evaluated exactly (``deviation_float32``: the reference subtracts float32 members in float32
and adds float32 probabilities in float32; ``deviation_float64``).  Counts and ROC tables have no tolerance.
"""

import math
import os
import warnings

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import probscores as restated

PATH = os.path.join(GOLDEN, "probscores_reference.npz")
DTYPES = ["float32", "float64"]
BINS = [10, 7]


@pytest.fixture(scope="module")
def golden():
    return np.load(PATH)


def crps_case_names():
    return [str(c) for c in np.load(PATH)["crps_cases"]]


def prob_case_names():
    return [str(c) for c in np.load(PATH)["prob_cases"]]


def within(got, want, bar):
    """NaN positions equal, exact zeros equal, everything else within ``bar`` relative; returns the worst deviation."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
    assert np.all(got[fin][want[fin] == 0] == 0.0)
    worst = float(np.max(np.abs(got[fin] - want[fin]) / np.where(want[fin] == 0, 1.0, np.abs(want[fin])), initial=0.0))
    assert worst <= bar, (worst, bar)
    return worst


def reldiag_object(golden, array, n_bins, min_count=10):
    """The reliability diagram object behind a golden array (4, n_bins)."""
    obj = {"X_min": float(golden["x_min"]), "bin_edges": golden["edges_b%d" % n_bins], "n_bins": n_bins, "min_count": min_count,
           "X_sum": np.array(array[0], dtype=np.float64)}
    for i, key in enumerate(restated.BIN_KEYS[1:], start=1):
        obj[key] = np.array(array[i], dtype=int)
    return obj


def roc_object(golden, array):
    obj = {"X_min": float(golden["x_min"]), "prob_thrs": golden["prob_thrs"]}
    for i, key in enumerate(restated.ROC_KEYS):
        obj[key] = np.array(array[i], dtype=int)
    return obj


def reldiag_array(obj):
    return np.stack([np.asarray(obj[k], dtype=np.float64) for k in restated.BIN_KEYS])


def roc_array(obj):
    return np.stack([obj[k] for k in restated.ROC_KEYS])


def typed(golden, name, dtype):
    return golden[name + "__p"].astype(dtype), golden[name + "__o"].astype(dtype)


@pytest.fixture
def host_kernel(monkeypatch):
    """The Python layer with tests/helpers/probscores.py in place of the two entry points: fields stay NumPy arrays."""
    from pysteps_amd.verification import probscores

    def crps_sums(dev_f, dev_o, planes, k, npix, shared):
        f = np.asarray(dev_f).reshape((1, k, npix) if shared else (planes, k, npix))
        o = np.asarray(dev_o).reshape(planes, npix)
        counts, sums = np.zeros(planes, np.uint64), np.zeros((planes, 2))
        for t in range(planes):
            counts[t], sums[t, 0], _ = restated.crps_terms(f[0 if shared else t], o[t])
        return counts, sums

    def bins(dev_p, dev_o, npix, x_min, edges, prob_thrs):
        # the kernel compares the widened values with the float64 numbers it is given
        counted = restated.bin_counts(np.asarray(dev_p, dtype=np.float64), np.asarray(dev_o, dtype=np.float64), x_min, edges, prob_thrs)
        out = [None, None, None]
        if edges is not None:
            out[0] = np.array([counted["count"], counted["events"]], dtype=np.uint64).T
            out[1] = np.array([counted["sum"], [0.0] * len(counted["sum"])]).T
        if prob_thrs is not None:
            out[2] = np.array(counted["roc"], dtype=np.uint64)
        return tuple(out)

    monkeypatch.setattr(probscores, "_upload", np.asarray)
    monkeypatch.setattr(probscores, "_crps_sums", crps_sums)
    monkeypatch.setattr(probscores, "_bins", bins)
    return probscores


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", crps_case_names())
def test_helper_reproduces_the_crps_goldens(golden, name, dtype):
    f, o = golden[name + "__f"].astype(dtype), golden[name + "__o"].astype(dtype)
    want = golden["%s__%s__crps" % (name, dtype)]
    n, total, magnitude = restated.crps_terms(f, o)
    assert n == int(want[1]) and magnitude >= abs(total)
    within(total, want[0], float(golden["deviation_" + dtype]))
    exact_n, exact = restated.crps_exact(f, o)
    assert exact_n == n
    within(float(exact), want[0], float(golden["deviation_" + dtype]))


def test_tie_pixels_by_hand():
    """K = 3, members 0.25, 0.5, 0.75: an observation equal to a member adds nothing from the two bins it touches."""
    f, o = restated.tie_pixels(3, np.float64)
    w = restated.crps_weights(3)
    per_pixel = [restated.crps_terms(f[:, :, i:i + 1], o[:, i:i + 1])[1] for i in range(9)]
    assert per_pixel[0] == 0.25 * w[2][1]  # obs = smallest: bin 1 touches it, bin 2 lies above the observation
    assert per_pixel[1] == 0.25 * w[1][0]  # obs = largest: bin 1 lies below the observation, bin 2 touches it
    assert per_pixel[2] == 0.0  # obs = the middle member of three: both inner bins touch it
    assert per_pixel[3] == 0.75 and per_pixel[4] == 0.0 and per_pixel[5] == 1.5  # all members 1.5; obs 0.75, 1.5, 3.0
    assert per_pixel[6] == math.fsum([0.25 * w[1][0], 0.125 * w[2][0], 0.125 * w[2][1]])  # obs 0.625 inside bin 2
    assert per_pixel[7] == math.fsum([0.25, 0.25 * w[1][1], 0.25 * w[2][1]])  # obs below all members
    assert per_pixel[8] == math.fsum([0.25 * w[1][0], 0.25 * w[2][0], 1.0])  # obs above all members
    f1, o1 = restated.tie_pixels(1, np.float64)  # one member: only the outer bins exist
    assert restated.crps_terms(f1, o1)[:2] == (9, math.fsum(abs(float(a) - float(b)) for a, b in zip(f1.ravel(), o1.ravel())))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", prob_case_names())
def test_helper_reproduces_the_binning_goldens(golden, name, dtype):
    p, o = typed(golden, name, dtype)
    x_min = float(golden["x_min"])
    for n_bins in BINS:
        counted = restated.bin_counts(p, o, x_min, edges=golden["edges_b%d" % n_bins])
        total = restated.add_to_reldiag(None, counted, 10)
        want = golden["%s__%s__b%d__reldiag" % (name, dtype, n_bins)]
        assert [total[k] for k in restated.BIN_KEYS[1:]] == want[1:].astype(int).tolist()
        within(restated.reldiag_x_sum(total), want[0], float(golden["deviation_" + dtype]))
    roc = restated.bin_counts(p, o, x_min, prob_thrs=golden["prob_thrs"])["roc"]
    assert roc == golden["%s__%s__roc" % (name, dtype)].T.tolist()


@pytest.mark.parametrize("dtype", DTYPES)
def test_min_count_applies_to_each_call(golden, dtype):
    """Nine pixels of a call add nothing, ten add their sums - in the helper as in the reference's objects."""
    x_min, edges = float(golden["x_min"]), golden["edges_b10"]
    calls = [restated.bin_counts(*typed(golden, name, dtype), x_min, edges=edges) for name in ("mincount_a", "mincount_b")]
    assert calls[0]["count"][:3] == [9, 10, 30] and calls[1]["count"][:2] == [10, 9] and calls[1]["count"][9] == 11
    total = restated.add_to_reldiag(None, calls[0], 10)
    assert total["num_idx"][:3] == [0, 10, 30] and total["Y_sum"][0] == 0 and not total["X_sum"][0]
    total = restated.add_to_reldiag(total, calls[1], 10)
    want = golden["mincount_ab__%s__b10__reldiag" % dtype]
    assert [total[k] for k in restated.BIN_KEYS[1:]] == want[1:].astype(int).tolist() and total["num_idx"][:2] == [10, 10]
    within(restated.reldiag_x_sum(total), want[0], float(golden["deviation_" + dtype]))


def test_edge_probabilities_fall_where_digitize_puts_them(golden):
    """0.0 and 1.0 lie inside the outer bins (the edges are -1e-6 and 1 + 1e-6); a probability on an edge belongs to the
    bin below it, its upper neighbour to the bin above, and what lies beyond the outer edges to no bin."""
    for n_bins in BINS:
        edges = golden["edges_b%d" % n_bins]
        o = np.ones(5)
        for j in range(n_bins + 1):
            p = np.array([edges[j], np.nextafter(edges[j], np.inf), np.nextafter(edges[j], -np.inf), 0.0, 1.0])
            count = restated.bin_counts(p, o, 0.5, edges=edges)["count"]
            want = [0] * n_bins
            for b in ([j - 1, j - 1] if j else []) + ([j] if j < n_bins else []) + [0, n_bins - 1]:
                want[b] += 1
            assert count == want
            assert count == np.bincount(np.digitize(p, edges, right=True), minlength=n_bins + 2)[1:n_bins + 1].tolist()


def test_compute_functions_return_the_references_bits(golden):
    from pysteps_amd.verification import probscores

    for dtype in DTYPES:
        for name in crps_case_names() + ["twocalls"]:
            row = golden["%s__%s__crps" % (name, dtype)]
            with np.errstate(all="ignore"):
                got = probscores.CRPS_compute({"CRPS_sum": np.float64(row[0]), "n": float(row[1])})
            assert np.array_equal(got, row[2], equal_nan=True)
        for name in prob_case_names() + ["mincount_ab"]:
            for n_bins in BINS:
                tag = "%s__%s__b%d" % (name, dtype, n_bins)
                with np.errstate(all="ignore"):
                    r, f = probscores.reldiag_compute(reldiag_object(golden, golden[tag + "__reldiag"], n_bins))
                assert np.array_equal(np.stack([r, f]), golden[tag + "__rf"], equal_nan=True)
            tag = "%s__%s" % (name, dtype)
            with np.errstate(all="ignore"):
                pofd, pod, area = probscores.ROC_curve_compute(roc_object(golden, golden[tag + "__roc"]), compute_area=True)
                short = probscores.ROC_curve_compute(roc_object(golden, golden[tag + "__roc"]))
            assert isinstance(pofd, list) and len(short) == 2 and short[1] == pod
            assert np.array_equal(np.array([pofd, pod]), golden[tag + "__curve"], equal_nan=True)
            assert np.array_equal(area, golden[tag + "__area"], equal_nan=True)
    assert np.isnan(golden["masked__float64__crps"][2]) and golden["masked__float64__crps"][1] == 0


def test_objects_have_the_references_keys_and_types(golden):
    from pysteps_amd.verification import probscores

    crps, rdiag, roc = probscores.CRPS_init(), probscores.reldiag_init(0.5, 7, 3), probscores.ROC_curve_init(0.5, 6)
    assert sorted(crps) == golden["crps_keys"].tolist() and crps == {"CRPS_sum": 0.0, "n": 0.0}
    assert sorted(rdiag) == golden["reldiag_keys"].tolist() and sorted(roc) == golden["roc_keys"].tolist()
    assert np.array_equal(rdiag["bin_edges"], golden["edges_b7"]) and rdiag["min_count"] == 3 and rdiag["n_bins"] == 7
    assert np.array_equal(probscores.reldiag_init(0.5)["bin_edges"], golden["edges_b10"])
    assert np.array_equal(probscores.ROC_curve_init(0.5)["prob_thrs"], golden["prob_thrs"]) and roc["prob_thrs"].size == 6
    assert rdiag["X_sum"].dtype == np.float64 and all(rdiag[k].dtype == np.dtype(int) for k in restated.BIN_KEYS[1:])
    assert all(roc[k].dtype == np.dtype(int) and roc[k].shape == (6,) for k in restated.ROC_KEYS)
    w = probscores.crps_weights(7)
    assert w.shape == (8, 2) and w.dtype == np.float64 and w.tolist() == [list(pair) for pair in restated.crps_weights(7)]
    assert w[7, 0] == 1.0 and w[0, 1] == 1.0 and w[0, 0] == 0.0 and w[7, 1] == 0.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_python_layer_fills_the_objects_as_the_reference_does(golden, host_kernel, dtype):
    ps = host_kernel
    bar = 5.0 * float(golden["deviation_" + dtype])  # derived quantities: the margin the GPU tests use
    crps = ps.CRPS_init()
    for name in ("quant_3", "quant_7"):
        f, o = golden[name + "__f"].astype(dtype), golden[name + "__o"].astype(dtype)
        before = f.copy()
        ps.CRPS_accum(crps, f, o)
        assert np.array_equal(f, before, equal_nan=True)  # the input is not modified
    want = golden["twocalls__%s__crps" % dtype]
    assert isinstance(crps["n"], float) and crps["n"] == want[1] and isinstance(crps["CRPS_sum"], np.float64)
    within(crps["CRPS_sum"], want[0], bar)
    within(ps.CRPS_compute(crps), want[2], bar)
    f, o = golden["masked__f"].astype(dtype), golden["masked__o"].astype(dtype)
    with pytest.warns(RuntimeWarning):
        assert np.isnan(ps.CRPS(f, o))  # n == 0: NaN and NumPy's warning, as in the reference
    table, obj = ps.crps_table(golden["quant_7__f"].astype(dtype), np.stack([golden["quant_7__o"].astype(dtype)] * 2), return_object=True)
    assert table.shape == (2,) and obj["n"].tolist() == [golden["quant_7__%s__crps" % dtype][1]] * 2
    within(table, [golden["quant_7__%s__crps" % dtype][2]] * 2, bar)
    assert ps.crps_table(golden["quant_7__f"].astype(dtype), golden["quant_7__o"].astype(dtype)).shape == ()
    for n_bins in BINS:
        rdiag = ps.reldiag_init(float(golden["x_min"]), n_bins)
        roc = ps.ROC_curve_init(float(golden["x_min"]))
        for name in ("mincount_a", "mincount_b"):
            ps.reldiag_accum(rdiag, *typed(golden, name, dtype))
            ps.ROC_curve_accum(roc, *typed(golden, name, dtype))
        want = golden["mincount_ab__%s__b%d__reldiag" % (dtype, n_bins)]
        assert np.array_equal(reldiag_array(rdiag)[1:], want[1:]) and all(rdiag[k].dtype == np.dtype(int) for k in restated.BIN_KEYS[1:])
        within(rdiag["X_sum"], want[0], bar)
        assert np.array_equal(roc_array(roc), golden["mincount_ab__%s__roc" % dtype])
    p, o = typed(golden, "k7", dtype)
    with np.errstate(all="ignore"):
        r, f = ps.reldiag(p, o, float(golden["x_min"]), n_bins=7)
        pofd, pod, area = ps.ROC_curve(p, o, float(golden["x_min"]), compute_area=True)
    within(np.stack([r, f]), golden["k7__%s__b7__rf" % dtype], bar)
    assert np.array_equal(np.array([pofd, pod]), golden["k7__%s__curve" % dtype], equal_nan=True) and area == golden["k7__%s__area" % dtype]
    both = (ps.reldiag_init(0.5, 7), ps.ROC_curve_init(0.5))
    ps._accum_both(both[0], both[1], p, o)
    within(np.stack(ps.reldiag_compute(both[0])), golden["k7__%s__b7__rf" % dtype], bar)
    assert np.array_equal(roc_array(both[1]), golden["k7__%s__roc" % dtype])


def test_threshold_types_decide_as_in_numpy(host_kernel):
    """On float32 observations a Python float ``X_min`` is compared as float32 and a numpy.float64 as float64."""
    ps = host_kernel
    o = np.full((3, 4), np.float32(0.1))
    p = np.full((3, 4), 0.5)
    for x_min, events in ((0.1, 12), (np.float64(0.1), 12), (np.float64(np.float32(0.1)) + 1e-12, 0)):
        roc = ps.ROC_curve_init(x_min, 3)
        ps.ROC_curve_accum(roc, p, o)
        assert int(roc["hits"][0]) == events and int(roc["hits"][0] + roc["false_alarms"][0]) == 12
    roc = ps.ROC_curve_init(np.float64(0.1), 3)
    ps.ROC_curve_accum(roc, p, np.full((3, 4), np.float32(0.099999994)))  # the float32 below float32(0.1) lies below 0.1
    assert int(roc["hits"][0]) == 0


def test_get_method_names_and_the_type_error():
    from pysteps_amd import verification
    from pysteps_amd.verification import probscores

    assert verification.get_method("crps", type="probabilistic") is probscores.CRPS
    assert verification.get_method("RelDiag", type="Probabilistic") is probscores.reldiag
    assert verification.get_method("roc", type="probabilistic") is probscores.ROC_curve
    assert verification.ProbScoresAccumulator.accepts_device and verification.crps_table is probscores.crps_table
    for name in probscores.__all__:
        assert name == "crps_weights" or getattr(verification, name) is getattr(probscores, name)
    with pytest.raises(ValueError, match="unknown probabilistic method rankhist"):
        verification.get_method("rankhist", type="probabilistic")
    with pytest.raises(ValueError, match=r"Unknown verification type ensemble\nThe available types are: \['deterministic', 'probabilistic'\]"):
        verification.get_method("rankhist", type="ensemble")
    assert callable(verification.get_method("csi"))  # the deterministic names are where they were


def test_objects_from_the_references_init_are_accepted(golden, host_kernel, ref_pysteps):
    from pysteps.verification import probscores as ref

    ps = host_kernel
    x_min = float(golden["x_min"])
    assert ps.CRPS_init() == ref.CRPS_init()
    for mine, theirs in ((ps.reldiag_init(x_min, 7, 4), ref.reldiag_init(x_min, 7, 4)), (ps.ROC_curve_init(x_min, 6), ref.ROC_curve_init(x_min, 6))):
        assert list(mine) == list(theirs)
        for key in theirs:
            assert np.array_equal(mine[key], theirs[key]) and type(mine[key]) is type(theirs[key])
            assert not isinstance(theirs[key], np.ndarray) or mine[key].dtype == theirs[key].dtype
    f, o = golden["rain_7__f"].astype(np.float64), golden["rain_7__o"].astype(np.float64)
    mine, theirs = ref.CRPS_init(), ref.CRPS_init()
    ps.CRPS_accum(mine, f, o)
    ref.CRPS_accum(theirs, f, o)
    assert mine["n"] == theirs["n"] and type(mine["n"]) is type(theirs["n"]) and type(mine["CRPS_sum"]) is type(theirs["CRPS_sum"])
    within(mine["CRPS_sum"], theirs["CRPS_sum"], 5.0 * float(golden["deviation_float64"]))
    ref.CRPS_accum(mine, f, o)  # and the reference takes the object back
    assert mine["n"] == 2 * theirs["n"]
    p, o = typed(golden, "k7", "float64")
    for n_bins in BINS:
        mine, theirs = ref.reldiag_init(x_min, n_bins), ref.reldiag_init(x_min, n_bins)
        ps.reldiag_accum(mine, p, o)
        ref.reldiag_accum(theirs, p, o)
        assert all(mine[k].dtype == theirs[k].dtype for k in restated.BIN_KEYS)
        assert np.array_equal(reldiag_array(mine)[1:], reldiag_array(theirs)[1:])
        within(mine["X_sum"], theirs["X_sum"], 5.0 * float(golden["deviation_float64"]))
        ref.reldiag_accum(mine, p, o)
        assert np.array_equal(mine["num_idx"], 2 * theirs["num_idx"])
    mine, theirs = ref.ROC_curve_init(x_min, 12), ref.ROC_curve_init(x_min, 12)
    ps.ROC_curve_accum(mine, p, o)
    ref.ROC_curve_accum(theirs, p, o)
    assert np.array_equal(roc_array(mine), roc_array(theirs)) and all(mine[k].dtype == theirs[k].dtype for k in restated.ROC_KEYS)
    with np.errstate(all="ignore"):
        assert ps.ROC_curve_compute(mine, True) == ref.ROC_curve_compute(theirs, True)


def test_declined_inputs_go_to_the_reference_with_a_warning(golden, host_kernel, ref_pysteps, monkeypatch):
    from pysteps.verification import probscores as ref

    from pysteps_amd.device import DeviceArray

    ps = host_kernel
    x_min = float(golden["x_min"])
    many, obs = restated.ensemble(65, 3, 4, 7, np.float64)
    with pytest.warns(RuntimeWarning, match="65 members .* running the reference's function"):
        assert ps.CRPS(many, obs) == ref.CRPS(many, obs)
    ints = (restated.ensemble(3, 3, 4, 8)[0] * 2).astype(np.int32)
    with pytest.warns(RuntimeWarning, match="dtype int32"):
        assert ps.CRPS(ints, ints[0]) == ref.CRPS(ints, ints[0])
    p, o = typed(golden, "k7", "float64")
    with np.errstate(all="ignore"):
        with pytest.warns(RuntimeWarning, match="65 bins"):
            got = ps.reldiag(p, o, x_min, n_bins=65)
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, ref.reldiag(p, o, x_min, n_bins=65)))
        with pytest.warns(RuntimeWarning, match="65 probability thresholds"):
            assert ps.ROC_curve(p, o, x_min, n_prob_thrs=65, compute_area=True) == ref.ROC_curve(p, o, x_min, n_prob_thrs=65, compute_area=True)
        with pytest.warns(RuntimeWarning, match="dtype float16"):
            got = ps.ROC_curve(p.astype(np.float16), o, x_min)
        assert got == ref.ROC_curve(p.astype(np.float16), o, x_min)
        with pytest.warns(RuntimeWarning, match="dtype int64"):
            ps.reldiag(p, np.nan_to_num(o, posinf=0, neginf=0).astype(np.int64), x_min)
        with warnings.catch_warnings():  # 64 of each are served: no warning
            warnings.simplefilter("error", RuntimeWarning)
            ps.reldiag_accum(ps.reldiag_init(x_min, 64), p, o)
            ps.ROC_curve_accum(ps.ROC_curve_init(x_min, 64), p, o)
            ps.CRPS_accum(ps.CRPS_init(), many[:64], obs)
    with pytest.raises(NotImplementedError):
        ps.crps_table(many, obs)
    with pytest.raises(ValueError):
        ps.crps_table(many[:3], obs[:2])
    with pytest.raises(ValueError):
        ps.reldiag_accum(ps.reldiag_init(x_min), p, o[:5])
    monkeypatch.setattr(ps, "lookup", lambda module, name, ours: None)  # pysteps is not importable: nothing to hand the input to
    with pytest.raises(NotImplementedError, match="65 members .* pysteps is not importable"):
        ps.CRPS(many, obs)
    with pytest.raises(NotImplementedError, match="dtype float16"):
        ps.reldiag(p.astype(np.float16), o, x_min)
    resident = DeviceArray((65, 3, 4), np.float64, ptr=8)  # a view of nothing: never read
    monkeypatch.undo()
    from pysteps_amd.verification import probscores

    with pytest.raises(NotImplementedError, match="65 members"):
        probscores.CRPS_accum(probscores.CRPS_init(), resident, DeviceArray((3, 4), np.float64, ptr=8))


def test_registration_is_opt_in(ref_pysteps):
    from pysteps.verification import probscores as ref

    from pysteps_amd import register
    from pysteps_amd._reference import lookup
    from pysteps_amd.verification import probscores

    def stock(name):
        return lookup("verification.probscores", name, getattr(probscores, name))

    def current():
        return tuple(getattr(ref, name) for name in probscores.SWAPPED)

    before = current()
    kept = (ref.CRPS_init, ref.CRPS_compute, ref.reldiag_init, ref.reldiag_compute, ref.ROC_curve_init, ref.ROC_curve_compute)
    try:
        added = register.register()
        assert current() == before and not [a for a in added if a.startswith("verification")]
        assert register.register(probscores=True)[-6:] == ["verification:" + name for name in probscores.SWAPPED]
        assert current() == tuple(getattr(probscores, name) for name in probscores.SWAPPED)
        assert kept == (ref.CRPS_init, ref.CRPS_compute, ref.reldiag_init, ref.reldiag_compute, ref.ROC_curve_init, ref.ROC_curve_compute)
        assert ref._reference_CRPS_accum is before[1] and stock("CRPS_accum") is before[1]
        assert stock("ROC_curve") is before[4]
        import pysteps.verification

        assert pysteps.verification.get_method("crps", type="probabilistic") is probscores.CRPS
        assert register.patch_probscores() == []  # already in place
        register.unpatch_probscores()
        assert current() == before and not [a for a in vars(ref) if a.startswith("_reference_")]
        assert stock("reldiag_accum") is before[3]
        register.unpatch_probscores()  # harmless when nothing is patched
        assert current() == before
    finally:
        register.unpatch_probscores()
        register.unregister_fft()
