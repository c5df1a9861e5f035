"""Ensemble skill and spread, host side (no GPU): the restatement of tests/helpers/ensscores.py against the goldens of
the unmodified reference, the ballot identity behind the categorical pair kernel, the pair order the shim and the
kernels share, the reference's checks and messages, and the Python layer with the restatement standing in for the
kernels.

Yardsticks.  Contingency tables of the pairs and categorical skill / spread: no tolerance.  Continuous scores: the
reference's own deviation from the restatement (``math.fsum`` sums, exact rationals), measured by
tools/make_golden_ensscores.py over every pair, member, skill and spread of the goldens: 2.32e-04 relative for float32
stacks (the reference forms residuals and means in float32, and ME cancels), 6.98e-14 for float64 stacks, 4.03e-16 for
the FSS.  The tests allow 5 x these.  Three results of the one-pixel float32 case (DRMSE per pair, skill and spread)
are NaN in the reference and zero by definition - its float32 ``mse - me**2`` rounds below zero; there a result is held
to the restatement (tests/helpers/ensscores.py ``held``).
"""

import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import detscores as det
from helpers import ensscores as restated
from test_detscores_cpu import host_kernel  # noqa: F401  (the stand-ins for psh_detcat_counts_dev / psh_detcont_sums_dev)

PATH = os.path.join(GOLDEN, "ensscores_reference.npz")
DTYPES = ["float32", "float64"]
METRICS = restated.metrics()


@pytest.fixture(scope="module")
def golden():
    return np.load(PATH)


def case_names():
    return [c[0] for c in restated.CASES]


def bar_of(golden, metric, dtype):
    """0 for a categorical metric, else 5 x the reference's measured deviation."""
    if metric in restated.CAT_METRICS:
        return 0.0
    return 5.0 * float(golden["deviation_fss" if metric == "fss" else "deviation_" + dtype])


def check_case(golden, name, dtype, skill, spread, pairs, tag=None, metrics=None):
    """``skill(metric, kwargs)``, ``spread(...)`` and ``pairs(...)`` of an implementation against one golden case;
    returns the worst relative deviation seen among the continuous scores."""
    key = "%s__%s__" % (name, dtype) + (tag or "")
    worst = 0.0
    for m, (label, metric, kwargs) in enumerate(metrics or METRICS):
        at = (lambda a: a) if tag else (lambda a: a[m])  # noqa: E731
        bar = bar_of(golden, metric, dtype)
        for what, fn in (("skill", skill), ("spread", spread), ("pairs", pairs)):
            if fn is None:
                continue
            with np.errstate(all="ignore"):
                got = fn(metric, kwargs)
            want, exact = at(golden[key + what]), at(golden[key + "exact_" + what])
            if metric in restated.CAT_METRICS:
                assert np.array_equal(got, want, equal_nan=True), (name, dtype, label, what)
            else:
                worst = max(worst, restated.held(got, want, exact, bar))
    return worst


def test_golden_covers_the_required_cases(golden):
    assert [str(c) for c in golden["cases"]] == case_names() and [str(v) for v in golden["labels"]] == [m[0] for m in METRICS]
    assert {c[1] for c in restated.CASES} == {2, 3, 5, 9} and {c[2] for c in restated.CASES} == {(1, 1), (7, 9), (33, 47), (64, 65)}
    assert {c[3] for c in restated.CASES} == set(restated.NAN_PATTERNS)
    assert {m[1] for m in METRICS} == {"CSI", "POD", "FAR", "BIAS", "RMSE", "MAE", "ME", "corr_p", "NMSE", "DRMSE", "RV", "beta1", "fss"}
    for name, K, shape, pattern in restated.CASES:
        x = golden[name + "__x"]
        assert x.shape == (K,) + shape and x.dtype == np.float32 and golden[name + "__o"].shape == shape
        nan = np.isnan(x)
        if pattern == "none":
            assert not nan.any()
        elif pattern == "border":
            assert nan[:, 0].all() and (K < 3 or shape[0] < 7 or nan[0].sum() < nan[2 if K > 2 else 1].sum())
        elif pattern == "allnan":
            assert nan[1].all() and not nan[0].any()
        else:
            assert (nan.sum(axis=0) == K - 1).sum() == 1 and nan.sum() == K - 1
    assert str(golden["conditioned_case"]) == restated.CONDITIONED_CASE
    assert 0.0 < float(golden["deviation_fss"]) < 1e-14 and 0.0 < float(golden["deviation_float64"]) < 1e-12 < float(golden["deviation_float32"]) < 1e-3
    assert abs(float(golden["deviation_float32"]) - 2.32e-04) < 1e-6 and abs(float(golden["deviation_float64"]) - 6.98e-14) < 1e-16
    assert abs(float(golden["deviation_fss"]) - 4.03e-16) < 1e-18 and int(golden["reference_lost"]) == 3  # the module docstring's
    assert os.path.getsize(PATH) < 512 * 1024


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", case_names())
def test_restatement_reproduces_the_goldens(golden, name, dtype):
    x, o = golden[name + "__x"].astype(dtype), golden[name + "__o"].astype(dtype)
    for t, thr in enumerate(restated.CAT_THRESHOLDS):
        want = [tuple(int(c) for c in row) for row in golden["%s__%s__tables" % (name, dtype)][t]]
        assert restated.ballot_tables(x, thr) == want and restated.direct_tables(x, thr) == want
    worst = check_case(golden, name, dtype, lambda m, kw: restated.ensemble_skill(x, o, m, **kw),
                       lambda m, kw: restated.ensemble_spread(x, m, **kw), lambda m, kw: restated.pair_scores(x, m, **kw))
    if name == restated.CONDITIONED_CASE:
        for c, (metric, kwargs) in enumerate(restated.CONDITIONED):
            worst = max(worst, check_case(golden, name, dtype, lambda m, kw: restated.ensemble_skill(x, o, m, **kw),
                                          lambda m, kw: restated.ensemble_spread(x, m, **kw),
                                          lambda m, kw: restated.pair_scores(x, m, **kw), "cond_%d__" % c, [(metric, metric, kwargs)]))
    for m, (label, metric, kwargs) in enumerate(METRICS):  # the stored restatement is this one
        np.testing.assert_array_equal(golden["%s__%s__exact_pairs" % (name, dtype)][m], restated.pair_scores(x, metric, **kwargs))
    print("%s %s: the reference's continuous scores within %.3g of the restatement" % (name, dtype, worst))


def test_ballot_identity_equals_direct_counting():
    rng = np.random.default_rng(5)
    stack = rng.gamma(0.8, 3.0, (7, 13, 21)).astype(np.float32)
    stack[rng.random(stack.shape) < 0.1] = np.nan
    stack[3] = np.nan
    for thr in (0.5, np.float64(0.1), -1.0, 1.0e6):
        tables = restated.ballot_tables(stack, thr)
        assert tables == restated.direct_tables(stack, thr) and len(tables) == 21
        assert all(sum(t) == 13 * 21 and min(t) >= 0 for t in tables)


def test_pair_table_is_the_references_loop_order():
    from pysteps_amd.verification import ensscores

    for K in range(2, 66):
        table = ensscores._pair_table(K)
        assert table.dtype == np.int32 and table.shape == (K * (K - 1) // 2, 2)
        assert [tuple(int(v) for v in row) for row in table] == restated.pair_order(K)


def test_checks_and_messages_equal_the_references(golden):
    """The checks run before any device call: no device is needed to see them."""
    from pysteps_amd.verification import ensscores

    x = golden[restated.CONDITIONED_CASE + "__x"].astype(np.float64)
    o = golden[restated.CONDITIONED_CASE + "__o"].astype(np.float64)
    messages = json.loads(str(golden["messages"]))
    calls = {"skill_2d": lambda: ensscores.ensemble_skill(x[0], o, "RMSE"), "spread_2d": lambda: ensscores.ensemble_spread(x[0], "RMSE"),
             "spread_one_member": lambda: ensscores.ensemble_spread(x[:1], "RMSE"),
             "skill_shape": lambda: ensscores.ensemble_skill(x, o[:, :5], "RMSE"),
             "spread_unknown": lambda: ensscores.ensemble_spread(x, "no_such_score")}
    assert sorted(calls) == sorted(k for k in messages if not k.endswith("lower_case"))
    for key, call in calls.items():
        with pytest.raises(ValueError) as exc:
            call()
        assert messages[key] == ["ValueError", str(exc.value)], key
    with pytest.raises(ValueError, match="must be greater than 1"):
        ensscores.pair_scores(x[:1], "RMSE")


def test_a_lower_case_metric_raises_the_references_keyerror(golden, host_kernel, host_pairs):  # noqa: F811
    x = golden[restated.CONDITIONED_CASE + "__x"].astype(np.float64)
    o = golden[restated.CONDITIONED_CASE + "__o"].astype(np.float64)
    messages = json.loads(str(golden["messages"]))
    with pytest.raises(KeyError) as exc:
        host_pairs.ensemble_skill(x, o, "rmse")
    assert messages["skill_lower_case"] == ["KeyError", str(exc.value)]
    with pytest.raises(KeyError) as exc:
        host_pairs.ensemble_spread(x, "csi", thr=0.5)
    assert messages["spread_lower_case"] == ["KeyError", str(exc.value)]
    with pytest.raises(KeyError):
        host_pairs.ensemble_spread(x, "Corr_P")


class _Reads(dict):
    """An error object that notes which moments a formula reads."""

    def __init__(self):
        super().__init__({k: np.float64(2.0) for k in det.MOMENTS + ["n"]})
        self.read = set()

    def __getitem__(self, key):
        self.read.add(key)
        return super().__getitem__(key)


def test_sum_mask_covers_what_the_formula_reads():
    from pysteps_amd.verification import detcontscores, ensscores

    served = [n for n in ensscores._CONTINUOUS if n not in ensscores._REFERENCE_ONLY]
    assert sorted(ensscores._SUM_MASK) == sorted(served)
    sums_of = {"me": {detcontscores._RES}, "mse": {detcontscores._RES2}, "mae": {detcontscores._ABS}, "mss": {detcontscores._SUM2},
               "cov": {detcontscores._OBS_PAIR, detcontscores._PRED_PAIR, detcontscores._OBS_PRED}}  # detcontscores._moments
    for name in served:
        err = _Reads()
        with np.errstate(invalid="ignore"):
            assert len(detcontscores.det_cont_fct_compute(err, [name])) == 1
        needed = set().union(*[sums_of.get(moment, set()) for moment in err.read])
        mask = ensscores._SUM_MASK[name]
        assert 0 < mask <= ensscores.FULL_MASK and needed == {s for s in range(7) if mask >> s & 1}, name
    assert {bin(m).count("1") for m in ensscores._SUM_MASK.values()} == {1, 2, 3}  # both tile sizes are in use


class _HostStack:
    """What the layer needs of an uploaded stack, on the host."""

    def __init__(self, a):
        self._a, self.shape, self.dtype = a, a.shape, a.dtype

    def view(self, i):
        return self._a[i]

    def __array__(self, dtype=None, copy=None):
        return self._a if dtype is None else self._a.astype(dtype)


@pytest.fixture
def host_pairs(monkeypatch, host_kernel):  # noqa: F811
    """The Python layer with tests/helpers in place of the two pair entry points: hits and events from packed event
    bits, the selected pair sums from ``math.fsum`` (hi) with a zero low word."""
    from pysteps_amd.verification import ensscores

    def planes(stack, K, npix):
        return np.asarray(stack).reshape(K, npix)

    def cat_pairs(stack, K, npix, thrs):
        x = planes(stack, K, npix).astype(np.float64)
        hits, events = np.zeros((len(thrs), K * (K - 1) // 2), np.uint64), np.zeros((len(thrs), K), np.uint64)
        for t, thr in enumerate(thrs):
            tables = restated.ballot_tables(x, np.float64(thr))
            hits[t] = [table[0] for table in tables]
            events[t] = restated.events(x, np.float64(thr)).sum(axis=1)
        return hits, events

    def cont_pairs(stack, K, npix, sum_mask):
        x = planes(stack, K, npix)
        counts, sums = np.zeros(K * (K - 1) // 2, np.uint64), np.zeros((K * (K - 1) // 2, 7, 2))
        for p, (i, j) in enumerate(restated.pair_order(K)):
            c, s, _ = det.raw_sums(x[i], x[j])
            counts[p] = c[2]
            for k in range(7):
                if sum_mask >> k & 1:
                    sums[p, k, 0] = s[det.SUMS[k]]
        return counts, sums

    monkeypatch.setattr(ensscores, "_cat_pairs", cat_pairs)
    monkeypatch.setattr(ensscores, "_cont_pairs", cont_pairs)
    monkeypatch.setattr(ensscores, "_upload", lambda X: _HostStack(np.asarray(X)))
    return ensscores


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", case_names())
def test_python_layer_scores_the_goldens(golden, host_pairs, name, dtype):
    """Routing, tables from hits and events, moments from pair and own sums, the mean in the reference's order: every
    golden case but the FSS (its sums are device work) through the restated kernels."""
    x, o = golden[name + "__x"].astype(dtype), golden[name + "__o"].astype(dtype)
    before = x.copy()
    metrics = [m for m in METRICS if m[1] != "fss"]
    indices = [i for i, m in enumerate(METRICS) if m[1] != "fss"]
    prefix = "%s__%s__" % (name, dtype)
    sub = {prefix + e + what: golden[prefix + e + what][indices] for e in ("", "exact_") for what in ("skill", "spread", "pairs")}
    view = _Sub(golden, sub)
    worst = check_case(view, name, dtype, lambda m, kw: host_pairs.ensemble_skill(x, o, m, **kw),
                       lambda m, kw: host_pairs.ensemble_spread(x, m, **kw), lambda m, kw: host_pairs.pair_scores(x, m, **kw),
                       metrics=metrics)
    if name == restated.CONDITIONED_CASE:
        for c, (metric, kwargs) in enumerate(restated.CONDITIONED):  # pair by pair through det_cont_fct
            worst = max(worst, check_case(golden, name, dtype, lambda m, kw: host_pairs.ensemble_skill(x, o, m, **kw),
                                          lambda m, kw: host_pairs.ensemble_spread(x, m, **kw),
                                          lambda m, kw: host_pairs.pair_scores(x, m, **kw), "cond_%d__" % c, [(metric, metric, kwargs)]))
    assert np.array_equal(x, before, equal_nan=True)
    print("%s %s: continuous skill, spread and pair scores within %.3g of the golden" % (name, dtype, worst))


class _Sub:
    """A golden file with some arrays replaced."""

    def __init__(self, golden, replaced):
        self._golden, self._replaced = golden, replaced

    def __getitem__(self, key):
        return self._replaced[key] if key in self._replaced else self._golden[key]


def test_declined_metrics_go_to_the_reference_with_a_warning(golden, host_pairs, ref_pysteps):
    from pysteps.verification import ensscores as ref

    x = golden["k3_7x9_border__x"].astype(np.float64)
    o = golden["k3_7x9_border__o"].astype(np.float64)
    clean = golden["k9_7x9_none__x"][:3].astype(np.float64)
    with np.errstate(all="ignore"):
        with pytest.warns(RuntimeWarning, match="the metric corr_s - running the reference's function"):
            got = host_pairs.ensemble_spread(clean, "corr_s")
        assert got == ref.ensemble_spread(clean, "corr_s")
        with pytest.warns(RuntimeWarning, match="the metric scatter"):
            assert host_pairs.ensemble_skill(clean, o, "scatter") == ref.ensemble_skill(clean, o, "scatter")
        ints = np.nan_to_num(x).astype(np.int32)
        with pytest.warns(RuntimeWarning, match="dtype int32"):
            assert host_pairs.ensemble_spread(ints, "CSI", thr=1) == ref.ensemble_spread(ints, "CSI", thr=1)
        many = np.tile(np.nan_to_num(x), (22, 1, 1))[:65]
        with pytest.warns(RuntimeWarning, match="65 members"):
            assert host_pairs.ensemble_spread(many, "MAE") == ref.ensemble_spread(many, "MAE")
        inf = np.nan_to_num(x)
        inf[1, 2, 3] = np.inf
        with pytest.warns(RuntimeWarning, match="an infinite value"):
            got = host_pairs.ensemble_spread(inf, "RMSE")
        assert np.array_equal(got, ref.ensemble_spread(inf, "RMSE"), equal_nan=True)
        with pytest.warns(RuntimeWarning, match="an infinite value"):
            got = host_pairs.ensemble_skill(inf, o, "MAE")
        assert np.array_equal(got, ref.ensemble_skill(inf, o, "MAE"), equal_nan=True)
    with pytest.raises(NotImplementedError, match="the metric sal"):
        host_pairs.pair_scores(x, "sal")


def test_exports_and_registration_are_opt_in(ref_pysteps):
    from pysteps.verification import ensscores as ref
    from pysteps.verification.interface import get_method

    from pysteps_amd import register, verification
    from pysteps_amd.verification import ensscores

    assert verification.ensemble_spread is ensscores.ensemble_spread and verification.SpreadSkillAccumulator.accepts_device
    assert verification.ensemble_skill is ensscores.ensemble_skill and verification.pair_scores is ensscores.pair_scores
    with pytest.raises(ValueError):
        verification.get_method("ens_spread", type="ensemble")  # reached through the module and the swap
    before = (ref.ensemble_skill, ref.ensemble_spread, ref.rankhist)
    try:
        added = register.register()
        assert (ref.ensemble_skill, ref.ensemble_spread) == before[:2] and "verification:ensemble_spread" not in added
        assert register.register(ensscores=True)[-2:] == ["verification:ensemble_skill", "verification:ensemble_spread"]
        assert ref.ensemble_spread is ensscores.ensemble_spread and ref.ensemble_skill is ensscores.ensemble_skill
        assert ref.rankhist is before[2] and ensscores._stock("ensemble_spread") is before[1]
        assert get_method("ens_spread", type="ensemble") is ensscores.ensemble_spread
        assert get_method("ens_skill", type="ensemble") is ensscores.ensemble_skill
        assert register.patch_ensscores() == []  # already in place
        register.unpatch_ensscores()
        assert (ref.ensemble_skill, ref.ensemble_spread, ref.rankhist) == before
        assert not [a for a in vars(ref) if a.startswith("_reference_")]
        register.unpatch_ensscores()  # harmless when nothing is patched
    finally:
        register.unpatch_ensscores()
        register.unregister_fft()
