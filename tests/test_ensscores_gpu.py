"""Ensemble skill and spread on the device (``pysteps_amd.verification.ensscores``, csrc/ensscores.hip).

Categorical skill, spread and pair scores are held to the goldens of the unmodified reference with no tolerance.
Continuous scores and the FSS are held to them within 5 x the reference's own deviation from the restatement of
tests/helpers/ensscores.py (2.32e-04 relative for float32 stacks, 6.98e-14 for float64 stacks, 4.03e-16 for the FSS:
tests/test_ensscores_cpu.py), NaN positions equal.  The raw output of the two pair kernels is held to the existing
per-member kernels bit for bit: every pair's seven sums and count to ``psh_detcont_sums_dev`` on (plane i, plane j),
every pair's table to ``psh_detcat_counts_dev``.
"""

import contextlib
import os
import warnings

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import ensscores as restated
from test_ensscores_cpu import DTYPES, METRICS, case_names, check_case

pytestmark = pytest.mark.gpu

PATH = os.path.join(GOLDEN, "ensscores_reference.npz")
# (shape, dtype, K, NaN pattern): one pixel; partial and full ballot steps; npix % 4 != 0, so members 1 and 2 are not
# 16-byte aligned and take the element path; K no multiple of either tile side, diagonal and off-diagonal tiles; the cap
# of 64 members, 32 pairs per lane; more chunks than 512 workgroups x 256 threads, so the grid stride runs
RAW_CASES = [((1, 1), "float32", 2, "none"), ((1, 63), "float32", 3, "onepixel"), ((1, 64), "float64", 3, "none"),
             ((1, 65), "float32", 4, "allnan"), ((33, 47), "float32", 3, "border"), ((257, 129), "float64", 5, "border"),
             ((257, 129), "float64", 9, "onepixel"), ((64, 64), "float32", 64, "allnan"), ((1226, 761), "float32", 4, "border")]


@pytest.fixture(scope="module")
def golden():
    return np.load(PATH)


@contextlib.contextmanager
def no_fallback():
    """Inside: a call that goes to the reference's function is an error."""
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*running the reference's function")
        yield


@pytest.mark.parametrize("resident", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", case_names())
def test_goldens(golden, name, dtype, resident):
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.verification import ensscores

    x, o = golden[name + "__x"].astype(dtype), golden[name + "__o"].astype(dtype)
    before = x.copy()
    X, O = (DeviceArray.from_host(x), DeviceArray.from_host(o)) if resident else (x, o)
    with no_fallback():
        worst = check_case(golden, name, dtype, lambda m, kw: ensscores.ensemble_skill(X, O, m, **kw),
                           lambda m, kw: ensscores.ensemble_spread(X, m, **kw), lambda m, kw: ensscores.pair_scores(X, m, **kw))
        if name == restated.CONDITIONED_CASE:  # conditioning is served on the device, pair by pair
            for c, (metric, kwargs) in enumerate(restated.CONDITIONED):
                worst = max(worst, check_case(golden, name, dtype, lambda m, kw: ensscores.ensemble_skill(X, O, m, **kw),
                                              lambda m, kw: ensscores.ensemble_spread(X, m, **kw),
                                              lambda m, kw: ensscores.pair_scores(X, m, **kw), "cond_%d__" % c,
                                              [(metric, metric, kwargs)]))
    print("%s %s: continuous and FSS skill, spread and pair scores within %.3g of the golden (bars %.3g, FSS %.3g)"
          % (name, dtype, worst, 5.0 * float(golden["deviation_" + dtype]), 5.0 * float(golden["deviation_fss"])))
    assert np.array_equal(x, before, equal_nan=True)  # the input is not modified
    if resident:
        assert np.array_equal(X.to_host(), before, equal_nan=True)


def per_member_kernels(host, dev, thrs):
    """What the existing kernels return for (plane i, plane j) of every pair: ``(counts (P, 4), sums (P, 11, 2), tables
    (P, nthr, 4))``.  Small ensembles go pair by pair on the planes where they lie; larger ones as two gathered stacks of
    P planes in one call (the planes then lie elsewhere, which must not matter)."""
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.verification import detcatscores, detcontscores

    K, npix = host.shape[0], host.shape[1] * host.shape[2]
    order = restated.pair_order(K)
    if K <= 9:
        counts, sums, tables = [], [], []
        for i, j in order:
            c, s = detcontscores._sums(dev.view(i), dev.view(j), 1, npix, True, 0, 0.0, 0.0)
            counts.append(c[0]), sums.append(s[0])
            tables.append(detcatscores._counts(dev.view(i), dev.view(j), 1, npix, True, thrs, thrs)[0])
        return np.stack(counts), np.stack(sums), np.stack(tables)
    F = DeviceArray.from_host(np.ascontiguousarray(host[[i for i, _ in order]]))
    O = DeviceArray.from_host(np.ascontiguousarray(host[[j for _, j in order]]))
    counts, sums = detcontscores._sums(F, O, len(order), npix, False, 0, 0.0, 0.0)
    return counts, sums, detcatscores._counts(F, O, len(order), npix, False, thrs, thrs)


@pytest.mark.parametrize("shape,dtype,K,pattern", RAW_CASES, ids=["%dx%d-%s-k%d" % (c[0] + (c[1], c[2])) for c in RAW_CASES])
def test_pair_kernels_return_the_bits_of_the_per_member_kernels(shape, dtype, K, pattern):
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.verification import detcontscores, ensscores

    host, _ = restated.members(K, shape[0], shape[1], 300 + K, dtype, pattern)
    dev = DeviceArray.from_host(host)
    npix = shape[0] * shape[1]
    # 9 thresholds cross the 8 of a pass; at 64 members a pass holds 4: 4 fill one, 5 cross it
    thr_sets = [[0.25 * t for t in range(4)], [0.25 * t for t in range(5)]] if K == 64 else [[0.25 * t for t in range(9)]]
    want_counts, want_sums, want_tables = per_member_kernels(host, dev, thr_sets[-1])
    counts, sums = ensscores._cont_pairs(dev, K, npix, ensscores.FULL_MASK)
    assert counts.dtype == np.uint64 and np.array_equal(counts, want_counts[:, 2])
    assert sums.shape == (len(counts), 7, 2) and sums.tobytes() == np.ascontiguousarray(want_sums[:, :7]).tobytes()
    # the members' own sums, which the Python layer joins to the pair sums, from one call with the stack on both sides
    own_counts, own_sums = ensscores._own(dev, K, npix)
    got_counts, got_sums = ensscores._pair_sums(counts, sums, own_counts, own_sums, K)
    assert np.array_equal(got_counts[:, :3], want_counts[:, :3]) and got_sums.tobytes() == want_sums.tobytes()
    assert detcontscores._OBS == 7 and not own_counts[:, 3].any()
    for thrs in thr_sets:
        hits, events = ensscores._cat_pairs(dev, K, npix, thrs)
        assert hits.shape == (len(thrs), len(counts)) and events.shape == (len(thrs), K)
        for t in range(len(thrs)):
            table = ensscores._pair_tables(hits[t], events[t], npix, K)
            got = np.stack([table[k] for k in ("hits", "misses", "false_alarms", "correct_negatives")], axis=1)
            assert np.array_equal(got, want_tables[:, t].astype(int)), (t, thrs[t])


@pytest.mark.parametrize("shape,dtype,K", [((33, 47), "float32", 3), ((257, 129), "float64", 5)])
def test_masked_calls_return_the_selected_sums_of_the_full_call(shape, dtype, K):
    """Every single sum (tile side 4, one slot), the two-sum masks (tile side 4, two slots), the three-sum mask and the
    others up to seven (tile side 2)."""
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.verification import ensscores

    host, _ = restated.members(K, shape[0], shape[1], 400 + K, dtype, "border")
    dev = DeviceArray.from_host(host)
    npix = shape[0] * shape[1]
    full_counts, full = ensscores._cont_pairs(dev, K, npix, ensscores.FULL_MASK)
    masks = [1 << s for s in range(7)] + sorted(set(ensscores._SUM_MASK.values())) + [0b0101101, 0b1111110]
    assert {bin(m).count("1") for m in masks} >= {1, 2, 3, 4, 6}
    for mask in masks:
        counts, sums = ensscores._cont_pairs(dev, K, npix, mask)
        assert np.array_equal(counts, full_counts)
        for s in range(7):
            want = full[:, s] if mask >> s & 1 else np.zeros_like(full[:, s])
            assert sums[:, s].tobytes() == np.ascontiguousarray(want).tobytes(), (mask, s)


def test_results_are_bit_identical_between_runs_and_positions():
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.verification import ensscores

    host, _ = restated.members(7, 61, 131, 500, np.float32, "border")  # 61 * 131 % 4 = 3
    npix, thrs = 61 * 131, [0.5, 2.0]
    whole, part = DeviceArray.from_host(host), DeviceArray.from_host(np.ascontiguousarray(host[2:5]))
    first = ensscores._cont_pairs(whole, 7, npix, ensscores.FULL_MASK) + ensscores._cat_pairs(whole, 7, npix, thrs)
    again = ensscores._cont_pairs(whole, 7, npix, ensscores.FULL_MASK) + ensscores._cat_pairs(whole, 7, npix, thrs)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
    counts, sums = ensscores._cont_pairs(part, 3, npix, ensscores.FULL_MASK)
    hits, events = ensscores._cat_pairs(part, 3, npix, thrs)
    order = restated.pair_order(7)
    rows = [order.index((i + 2, j + 2)) for i, j in restated.pair_order(3)]
    assert counts.tobytes() == first[0][rows].tobytes() and sums.tobytes() == np.ascontiguousarray(first[1][rows]).tobytes()
    assert np.array_equal(hits, first[2][:, rows]) and np.array_equal(events, first[3][:, 2:5])


def test_decline_paths(golden, ref_pysteps):
    from pysteps.verification import ensscores as ref

    from pysteps_amd.device import DeviceArray
    from pysteps_amd.verification import ensscores

    x = golden["k9_7x9_none__x"].astype(np.float64)
    o = golden["k9_7x9_none__o"].astype(np.float64)
    many = np.tile(x, (8, 1, 1))[:65]
    ints = x.astype(np.int32)
    inf = x.copy()
    inf[1, 2, 3] = np.inf
    with np.errstate(all="ignore"):
        for why, stack, metric, kwargs in (("65 members", many, "MAE", {}), ("dtype int32", ints, "CSI", {"thr": 1}),
                                           ("an infinite value", inf, "RMSE", {}), ("the metric corr_s", x, "corr_s", {})):
            with pytest.warns(RuntimeWarning, match=why + ".* - running the reference's function"):
                got = ensscores.ensemble_spread(stack, metric, **kwargs)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                assert np.array_equal(got, ref.ensemble_spread(stack, metric, **kwargs), equal_nan=True), why
            with pytest.warns(RuntimeWarning, match=why):
                got = ensscores.ensemble_skill(stack, o.astype(stack.dtype), metric, **kwargs)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                assert np.array_equal(got, ref.ensemble_skill(stack, o.astype(stack.dtype), metric, **kwargs), equal_nan=True), why
            if stack.dtype == np.float64:
                with pytest.raises(NotImplementedError, match=why):
                    ensscores.ensemble_spread(DeviceArray.from_host(stack), metric, **kwargs)
                with pytest.raises(NotImplementedError, match=why):
                    ensscores.ensemble_skill(DeviceArray.from_host(stack), DeviceArray.from_host(o), metric, **kwargs)
        # conditioning and the FSS are served on the device: no warning, resident stacks welcome
        with no_fallback():
            dev = DeviceArray.from_host(x)
            assert np.isfinite(ensscores.ensemble_spread(dev, "RMSE", conditioning="single", thr=0.5))
            assert np.isfinite(ensscores.ensemble_spread(dev, "fss", thr=0.5, scale=3))
            assert np.array_equal(ensscores.ensemble_spread(inf, "CSI", thr=0.5), ref.ensemble_spread(inf, "CSI", thr=0.5))


def test_accumulator_equals_direct_calls(golden):
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.verification import SpreadSkillAccumulator, ensscores

    x, o = golden["k9_33x47_border__x"], golden["k9_33x47_border__o"]
    leads = [np.ascontiguousarray(x[3 * t:3 * t + 3]) for t in range(3)]
    obs = np.stack([o, np.roll(o, 1, axis=0), np.roll(o, 2, axis=1)])
    metrics = ["CSI", "RMSE", "corr_p", "FAR"]
    for resident in (True, False):
        acc = SpreadSkillAccumulator(obs, metrics, thr=0.5)
        assert acc.accepts_device
        for members in leads:
            acc(DeviceArray.from_host(members) if resident else members)
        assert acc.received == [DeviceArray if resident else np.ndarray] * 3 and acc.n_leadtimes == 3
        assert acc.skill.shape == (3, 4) and acc.spread.shape == (3, 4)
        with np.errstate(all="ignore"):
            for t, members in enumerate(leads):
                for m, metric in enumerate(metrics):
                    kwargs = {"thr": 0.5} if metric in ("CSI", "FAR") else {}
                    assert np.array_equal(acc.skill[t, m], ensscores.ensemble_skill(members, obs[t], metric, **kwargs), equal_nan=True)
                    assert np.array_equal(acc.spread[t, m], ensscores.ensemble_spread(members, metric, **kwargs), equal_nan=True)
        with pytest.raises(ValueError):
            acc(leads[0])  # a fourth lead time without an observation
    with pytest.raises(ValueError):
        SpreadSkillAccumulator(obs, ["CSI"])  # a categorical metric without a threshold


def test_accumulator_inside_a_real_steps_run(ref_pysteps):
    """The real pysteps.nowcasts.steps with the resident loop and return_output=False: the accumulator receives the
    members where they lie and no member is downloaded."""
    from pysteps import nowcasts

    from pysteps_amd import register
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.nowcasts import utils as loop
    from pysteps_amd.verification import SpreadSkillAccumulator
    from test_callers_gpu import _steps_inputs, _steps_kwargs

    frames, V = _steps_inputs(256, 256)
    kw = _steps_kwargs()
    n_leadtimes = 3
    observations = np.stack([np.roll(frames[-1], (2 * (t + 1), 3 * (t + 1)), axis=(0, 1)) for t in range(n_leadtimes)])
    steps = nowcasts.get_method("steps")
    try:
        register.register(patch_main_loop=True)
        acc = SpreadSkillAccumulator(DeviceArray.from_host(observations), ["CSI", "RMSE"], thr=0.0)  # dBR
        out = steps(frames, V, n_leadtimes, extrap_method="semilagrangian_hip", callback=acc, return_output=False, **kw)
        assert out is None and "download" not in loop.last_run_stats and "callback" in loop.last_run_stats
        assert acc.n_leadtimes == n_leadtimes and acc.received == [DeviceArray] * n_leadtimes
        assert acc.skill.shape == (n_leadtimes, 2) and acc.spread.shape == (n_leadtimes, 2)
        assert np.isfinite(acc.skill).all() and np.isfinite(acc.spread).all()
        assert 0.0 < acc.skill[:, 0].min() and acc.skill[:, 0].max() <= 1.0 and 0.0 < acc.spread[:, 0].min() and acc.spread[:, 0].max() <= 1.0
        assert acc.skill[:, 1].min() > 0.0 and acc.spread[:, 1].min() > 0.0
    finally:
        register.unpatch_main_loop()
        register.unregister_fft()


def test_registered_reference_functions_run_on_the_device(golden, ref_pysteps):
    from pysteps.verification import ensscores as ref
    from pysteps.verification.interface import get_method

    from pysteps_amd import register
    from pysteps_amd.verification import ensscores

    name, dtype = "k5_33x47_none", "float64"
    x, o = golden[name + "__x"].astype(dtype), golden[name + "__o"].astype(dtype)
    stock = (ref.ensemble_skill, ref.ensemble_spread, ref.rankhist)
    try:
        assert register.register(ensscores=True)[-2:] == ["verification:ensemble_skill", "verification:ensemble_spread"]
        assert ref.ensemble_spread is ensscores.ensemble_spread and ref.ensemble_skill is ensscores.ensemble_skill
        assert ref.rankhist is stock[2]
        assert get_method("ens_spread", type="ensemble") is ensscores.ensemble_spread
        assert register.patch_ensscores() == []  # a second patch finds them in place
        with no_fallback():
            check_case(golden, name, dtype, lambda m, kw: get_method("ens_skill", type="ensemble")(x, o, m, **kw),
                       lambda m, kw: get_method("ens_spread", type="ensemble")(x, m, **kw), None)
        with pytest.warns(RuntimeWarning, match="the metric scatter"):  # the parked stock function takes what is declined
            assert ref.ensemble_spread(x, "scatter") == stock[1](x, "scatter")
    finally:
        register.unpatch_ensscores()
        register.unregister_fft()
    assert (ref.ensemble_skill, ref.ensemble_spread, ref.rankhist) == stock
    assert not [a for a in vars(ref) if a.startswith("_reference_")]


def test_entry_points_refuse_with_an_error_code():
    from pysteps_amd import _lib
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.verification import ensscores

    stack = DeviceArray.from_host(np.zeros((3, 8, 9), np.float32))
    hits, events = DeviceArray((1, 3), np.uint64), DeviceArray((1, 3), np.uint64)
    counts, sums = DeviceArray((3,), np.uint64), DeviceArray((3, 7, 2), np.float64)
    thr = np.array([0.5])
    lib = _lib.lib()
    for K in (1, 65):  # fewer than a pair, more than the cap
        assert lib.psh_detcat_pairs_dev(stack.ptr, 0, K, 72, thr.ctypes.data, 1, hits.ptr, events.ptr) != 0
        assert lib.psh_detcont_pairs_dev(stack.ptr, 0, K, 72, 127, counts.ptr, sums.ptr) != 0
    assert lib.psh_detcat_pairs_dev(stack.ptr, 0, 3, 72, thr.ctypes.data, 0, hits.ptr, events.ptr) != 0  # no threshold
    assert lib.psh_detcat_pairs_dev(None, 0, 3, 72, thr.ctypes.data, 1, hits.ptr, events.ptr) != 0
    assert lib.psh_detcat_pairs_dev(stack.ptr, 0, 3, 72, None, 1, hits.ptr, events.ptr) != 0
    assert lib.psh_detcat_pairs_dev(stack.ptr, 0, 3, 72, thr.ctypes.data, 1, None, events.ptr) != 0
    assert lib.psh_detcont_pairs_dev(None, 0, 3, 72, 127, counts.ptr, sums.ptr) != 0
    assert lib.psh_detcont_pairs_dev(stack.ptr, 0, 3, 72, 127, counts.ptr, None) != 0
    assert lib.psh_detcont_pairs_dev(stack.ptr, 0, 3, 0, 127, counts.ptr, sums.ptr) != 0  # no pixel
    assert lib.psh_detcont_pairs_dev(stack.ptr + 2, 0, 3, 72, 127, counts.ptr, sums.ptr) != 0  # not aligned to an element
    for mask in (0, 128):
        assert lib.psh_detcont_pairs_dev(stack.ptr, 0, 3, 72, mask, counts.ptr, sums.ptr) != 0
    with pytest.raises(ValueError):
        ensscores._cat_pairs(stack, 1, 72, [0.5])
    # refused calls launch nothing: the stack still counts as before
    assert ensscores._cat_pairs(stack, 3, 72, [-1.0, 0.0])[0].tolist() == [[72, 72, 72], [0, 0, 0]]
