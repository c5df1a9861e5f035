"""The fractions skill score's host side (no GPU): the integer restatement against the reference's goldens and against
SciPy's filter, the Python layer (objects, messages, fall-back, accumulator, registration) with the restatement standing
in for the kernel.

Yardstick: tests/helpers/fss.py counts the three sums behind the score as integers.  The reference computes them by
float filtering, so it deviates from the integers; tools/make_golden_fss.py measured that deviation over the committed
cases (``deviation_sums`` relative on a sum, ``deviation_fss`` absolute on a score, stored in
tests/golden/fss_reference.npz) and the tests allow 5 x it, the project's standing rule.  The device is held to the same
integers with no tolerance in tests/test_fss_gpu.py.
"""

import json
import os
import warnings

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import fss as restated

PATH = os.path.join(GOLDEN, "fss_reference.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(PATH)


def case_names():
    return [str(c) for c in np.load(PATH)["cases"]]


def bars(golden):
    return 5.0 * float(golden["deviation_sums"]), 5.0 * float(golden["deviation_fss"])


def thresholds_of(golden):
    return [float(t) for t in golden["thresholds"]]  # Python floats, as the golden run used


@pytest.fixture
def host_kernel(monkeypatch):
    """The Python layer with tests/helpers/fss.py in place of psh_fss_sums_dev: fields stay NumPy arrays, thresholds
    arrive as the float64 numbers to compare with."""
    from pysteps_amd.verification import spatialscores

    def sums(dev_f, dev_o, K, m, n, shared, thr_f, thr_o, scales):
        f = np.asarray(dev_f, dtype=np.float64).reshape(K, m, n)
        o = np.asarray(dev_o, dtype=np.float64).reshape((m, n) if shared else (K, m, n))
        out = np.empty((K, len(thr_f), len(scales), 3), dtype=np.uint64)
        for k in range(K):
            ok = o if shared else o[k]
            for i, (tf, to) in enumerate(zip(thr_f, thr_o)):
                bf, bo = restated.indicator(f[k], np.float64(tf)), restated.indicator(ok, np.float64(to))
                for j, s in enumerate(scales):
                    cf, co = restated.window_counts(bf, s), restated.window_counts(bo, s)
                    out[k, i, j] = [(cf * cf).sum(), (cf * co).sum(), (co * co).sum()]
        return out

    monkeypatch.setattr(spatialscores, "_sums", sums)
    monkeypatch.setattr(spatialscores, "_upload", lambda X: np.asarray(X))
    return spatialscores


def test_golden_covers_the_required_cases(golden):
    shapes = {tuple(golden[name + "__f"].shape) for name in case_names()}
    assert {(257, 311), (640, 710), (1024, 1024)} <= shapes
    assert [int(s) for s in golden["scales"]] == [1, 2, 3, 8, 16, 33, 64, 128, 255] and len(golden["thresholds"]) == 3
    f = golden["p640x710__f"]
    assert f.dtype == np.float32 and np.isnan(f).any() and np.isposinf(f).any() and np.isneginf(f).any()
    assert (f == np.float32(0.7)).any() and 0.7 in thresholds_of(golden)
    assert np.isnan(golden["dry64x80__float32__fss"]).all() and np.isnan(golden["dry64x80__float64__fss"]).all()
    assert np.all(golden["same129x140__float32__fss"] == 1.0) and np.all(golden["same129x140__float64__fss"] == 1.0)
    # the two dtypes differ where the threshold lies in the rounding gap of a value of the field
    assert not np.array_equal(golden["p640x710__float32__sums"][1], golden["p640x710__float64__sums"][1])
    assert 0.0 < float(golden["deviation_sums"]) < 1e-12 and 0.0 < float(golden["deviation_fss"]) < 1e-12


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("name", case_names())
def test_restatement_reproduces_the_reference(golden, name, dtype):
    bar_sums, bar_fss = bars(golden)
    f, o = golden[name + "__f"].astype(dtype), golden[name + "__o"].astype(dtype)
    thrs, scales = thresholds_of(golden), [int(s) for s in golden["scales"]]
    exact = restated.sums_table(f, o, thrs, scales)
    want_sums, want_fss = golden["%s__%s__sums" % (name, dtype)], golden["%s__%s__fss" % (name, dtype)]
    worst_sum = worst_fss = 0.0
    for i in range(len(thrs)):
        for j, scale in enumerate(scales):
            got = restated.as_float_sums(exact[i, j], scale)
            for g, w in zip(got, want_sums[i, j]):
                if g == 0.0:
                    assert w == 0.0
                else:
                    worst_sum = max(worst_sum, abs(float(w) - float(g)) / float(g))
            s = restated.score(exact[i, j], scale)
            assert np.isnan(s) == np.isnan(want_fss[i, j])
            if not np.isnan(s):
                worst_fss = max(worst_fss, abs(float(s) - float(want_fss[i, j])))
            if name.startswith("same"):
                assert s == 1.0
            if name.startswith("dry"):
                assert np.isnan(s)
    print("%s %s: sums within %.3g (bar %.3g), FSS within %.3g (bar %.3g)" % (name, dtype, worst_sum, bar_sums, worst_fss, bar_fss))
    assert worst_sum <= bar_sums and worst_fss <= bar_fss


@pytest.mark.parametrize("s", range(1, 10))
def test_window_placement_equals_scipy(s):
    from scipy.ndimage import uniform_filter

    rng = np.random.default_rng(s)
    binary = rng.random((23, 31)) < 0.4
    want = uniform_filter(binary.astype(float), size=s, mode="constant", cval=0.0) * s * s
    got = restated.window_counts(binary, s)
    assert np.array_equal(got, np.rint(want).astype(np.int64)) and np.max(np.abs(want - np.rint(want))) < 1e-9
    # every window by brute force as well
    a = s // 2
    for y, x in ((0, 0), (22, 30), (11, 7), (1, 29)):
        assert got[y, x] == binary[max(y - a, 0):max(y - a + s, 0), max(x - a, 0):max(x - a + s, 0)].sum()


def test_objects_messages_and_merge_equal_the_references(golden):
    from pysteps_amd.verification import spatialscores

    obj = spatialscores.fss_init(0.5, 4)
    assert sorted(obj) == [str(k) for k in golden["keys"]]
    assert obj == dict(thr=0.5, scale=4, sum_fct_sq=0.0, sum_fct_obs=0.0, sum_obs_sq=0.0)
    messages = json.loads(str(golden["messages"]))
    with pytest.raises(ValueError) as exc:
        spatialscores.fss_accum(spatialscores.fss_init(1.0, 2), np.zeros((4, 5)), np.zeros((5, 4)))
    assert str(exc.value) == messages["shape"]
    with pytest.raises(ValueError) as exc:
        spatialscores.fss_accum(spatialscores.fss_init(1.0, 2), np.zeros((2, 4, 5)), np.zeros((2, 4, 5)))
    assert str(exc.value) == messages["shape"]
    with pytest.raises(ValueError) as exc:
        spatialscores.fss_merge(spatialscores.fss_init(1.0, 2), spatialscores.fss_init(2.0, 2))
    assert str(exc.value) == messages["merge_thr"]
    with pytest.raises(ValueError) as exc:
        spatialscores.fss_merge(spatialscores.fss_init(1.0, 2), spatialscores.fss_init(1.0, 4))
    assert str(exc.value) == messages["merge_scale"]
    a = dict(thr=1.0, scale=2, sum_fct_sq=1.5, sum_fct_obs=0.5, sum_obs_sq=2.0)
    merged = spatialscores.fss_merge(a, dict(a, sum_fct_sq=0.25))
    assert merged == dict(a, sum_fct_sq=1.75, sum_fct_obs=1.0, sum_obs_sq=4.0) and a["sum_fct_sq"] == 1.5
    assert spatialscores.fss_compute(a) == 1.0 - (1.5 - 1.0 + 2.0) / 3.5


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_python_layer_scores_the_goldens(golden, host_kernel, dtype):
    """fss, fss_accum and fss_table through the restated kernel: what a threshold stands for against a float32 field,
    the division, the NaN of an all-dry pair (a RuntimeWarning like the reference's), exactly 1 for identical fields."""
    _, bar_fss = bars(golden)
    thrs, scales = thresholds_of(golden), [int(s) for s in golden["scales"]]
    for name in ("p257x311", "same129x140", "dry64x80"):
        f, o = golden[name + "__f"].astype(dtype), golden[name + "__o"].astype(dtype)
        want = golden["%s__%s__fss" % (name, dtype)]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            table, counts = host_kernel.fss_table(f, o, thrs, scales, return_sums=True)
        assert table.shape == (3, 9) and counts.shape == (3, 9, 3) and counts.dtype == np.uint64
        exact = restated.sums_table(f, o, thrs, scales)
        assert [[list(map(int, c)) for c in row] for row in counts] == [[list(c) for c in row] for row in exact]
        assert np.array_equal(np.isnan(table), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.max(np.abs(table[ok] - want[ok]), initial=0.0) <= bar_fss
        one = host_kernel.fss(f, o, thrs[1], scales[3]) if name != "dry64x80" else None
        if one is not None:
            assert isinstance(one, np.float64) and one == table[1, 3]
    with pytest.warns(RuntimeWarning):
        assert np.isnan(host_kernel.fss(np.zeros((64, 80), dtype), np.zeros((64, 80), dtype), 0.5, 8))
    f = golden["same129x140__f"].astype(dtype)
    assert host_kernel.fss(f, f.copy(), 0.7, 16) == 1.0
    stack = np.stack([golden["p257x311__f"], golden["p257x311__o"]]).astype(dtype)
    shared = host_kernel.fss_table(stack, stack[1], thrs, [2, 33])
    paired = host_kernel.fss_table(stack, stack[::-1].copy(), thrs, [2, 33])
    assert shared.shape == (2, 3, 2) and np.all(shared[1] == 1.0) and np.array_equal(shared[0], paired[0])
    assert np.array_equal(paired[0], paired[1])  # the score is symmetric in its two fields


def test_threshold_type_decides_as_in_numpy(golden, host_kernel):
    """float32(0.7) >= 0.7 holds for a Python float (compared as float32) and not for numpy.float64(0.7)."""
    f, o = golden["p257x311__f"], golden["p257x311__o"]
    _, as_python = host_kernel.fss_table(f, o, [0.7], [3], return_sums=True)
    _, as_f64 = host_kernel.fss_table(f, o, [np.float64(0.7)], [3], return_sums=True)
    assert list(map(int, as_python[0, 0])) == list(restated.sums(f, o, 0.7, 3))
    assert list(map(int, as_f64[0, 0])) == list(restated.sums(f, o, np.float64(0.7), 3))
    assert not np.array_equal(as_python, as_f64)
    _, wide = host_kernel.fss_table(f.astype(np.float64), o.astype(np.float64), [0.7], [3], return_sums=True)
    assert np.array_equal(wide, as_f64)


def test_objects_merge_with_the_references(golden, host_kernel, ref_pysteps):
    from pysteps.verification import spatialscores as ref

    bar_sums, bar_fss = bars(golden)
    f, o = golden["p257x311__f"].astype(np.float64), golden["p257x311__o"].astype(np.float64)
    mine, theirs = host_kernel.fss_init(0.5, 8), ref.fss_init(0.5, 8)
    host_kernel.fss_accum(mine, f, o)
    ref.fss_accum(theirs, f, o)
    assert sorted(mine) == sorted(theirs) and all(isinstance(mine[k], np.float64) for k in mine if k.startswith("sum"))
    for key in ("sum_fct_sq", "sum_fct_obs", "sum_obs_sq"):
        assert abs(mine[key] - theirs[key]) <= bar_sums * theirs[key]
    both = [ref.fss_merge(mine, theirs), host_kernel.fss_merge(theirs, mine), ref.fss_merge(theirs, theirs)]
    scores = [ref.fss_compute(both[0]), host_kernel.fss_compute(both[1]), host_kernel.fss_compute(both[2])]
    assert max(scores) - min(scores) <= bar_fss and 0.0 < scores[0] < 1.0
    host_kernel.fss_accum(theirs, f, o)  # an object the reference made and filled takes a pair from this side
    assert abs(ref.fss_compute(theirs) - scores[0]) <= bar_fss


def test_unsupported_inputs_go_to_the_reference_with_a_warning(golden, host_kernel, ref_pysteps):
    from pysteps.verification import spatialscores as ref

    f, o = golden["p257x311__f"], golden["p257x311__o"]
    for kwargs, fields in (({"thr": 1, "scale": 4}, (np.nan_to_num(f, posinf=0, neginf=0).astype(np.int32),
                                                     np.nan_to_num(o, posinf=0, neginf=0).astype(np.int32))),
                           ({"thr": 0.5, "scale": 300}, (f, o)), ({"thr": 1e30, "scale": 4}, (f, o))):
        with pytest.warns(UserWarning, match="running the reference's function"), np.errstate(all="ignore"):
            got = host_kernel.fss(fields[0], fields[1], kwargs["thr"], kwargs["scale"])
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            want = ref.fss(fields[0], fields[1], kwargs["thr"], kwargs["scale"])
        assert got == want or (np.isnan(got) and np.isnan(want))
    with pytest.raises(NotImplementedError):
        host_kernel.fss_table(f, o, [0.5], [300])
    with pytest.raises(NotImplementedError):
        host_kernel.fss_table(f, o, [0.5], [2.5])


def test_accumulator_on_host_stacks(golden, host_kernel, monkeypatch):
    """Without a loop that hands over device members the accumulator scores the host stack it receives: per lead time
    one object per threshold and scale, pooled over the members in member order like a loop of fss_accum."""
    from pysteps_amd.device import DeviceArray

    monkeypatch.setattr(DeviceArray, "from_host", classmethod(lambda cls, a, **kw: _HostPlanes(np.asarray(a))))
    f, o = golden["p257x311__f"].astype(np.float64), golden["p257x311__o"].astype(np.float64)
    obs = np.stack([o, np.roll(o, 4, axis=1)])
    leads = [np.stack([f, np.roll(f, 2, axis=0), o]), np.stack([np.roll(f, 1, axis=1), f, f])]
    thrs, scales = [0.5, 4.0], [1, 8, 33]
    acc = host_kernel.FssAccumulator(obs, thrs, scales, per_member=True)
    assert acc.accepts_device
    for members in leads:
        acc(members)
    assert acc.n_leadtimes == 2 and acc.received == [np.ndarray] * 2
    assert acc.fss.shape == (2, 2, 3) and acc.member_fss.shape == (2, 3, 2, 3)
    for t, members in enumerate(leads):
        for i, thr in enumerate(thrs):
            for j, scale in enumerate(scales):
                want = host_kernel.fss_init(thr, scale)
                for k in range(3):
                    host_kernel.fss_accum(want, members[k], obs[t])
                    assert acc.member_fss[t, k, i, j] == host_kernel.fss(members[k], obs[t], thr, scale)
                assert acc.objects[t][i][j] == want and acc.fss[t, i, j] == host_kernel.fss_compute(want)
    with pytest.raises(ValueError):
        acc(leads[0])  # a third lead time without an observation


class _HostPlanes:
    """What the accumulator needs of a DeviceArray, on the host."""

    def __init__(self, a):
        self._a, self.shape, self.dtype = a, a.shape, a.dtype

    def view(self, i):
        return self._a[i]


def test_get_method_resolves():
    from pysteps_amd import verification
    from pysteps_amd.verification import spatialscores

    assert verification.get_method("fss") is spatialscores.fss and verification.get_method("FSS") is spatialscores.fss
    with pytest.raises(ValueError):
        verification.get_method("sal")
    assert verification.FssAccumulator is spatialscores.FssAccumulator and verification.fss_table is spatialscores.fss_table


def test_registration_is_opt_in(ref_pysteps):
    from pysteps import verification as ref_verification
    from pysteps.verification import spatialscores as ref

    from pysteps_amd import register
    from pysteps_amd._reference import lookup
    from pysteps_amd.verification import spatialscores

    before = (ref.fss, ref.fss_accum)
    try:
        added = register.register()
        assert (ref.fss, ref.fss_accum) == before and not [a for a in added if a.startswith("verification")]
        assert ref_verification.get_method("fss") is before[0]
        assert register.register(fss=True)[-2:] == ["verification:fss", "verification:fss_accum"]
        assert ref.fss is spatialscores.fss and ref.fss_accum is spatialscores.fss_accum
        assert ref_verification.get_method("fss") is spatialscores.fss
        assert lookup("verification.spatialscores", "fss_accum", spatialscores.fss_accum) is before[1]
        assert register.patch_fss() == []  # already in place
        register.unpatch_fss()
        assert (ref.fss, ref.fss_accum) == before and ref_verification.get_method("fss") is before[0]
        assert not hasattr(ref, "_reference_fss") and not hasattr(ref, "_reference_fss_accum")
        assert lookup("verification.spatialscores", "fss_accum", spatialscores.fss_accum) is before[1]
        register.unpatch_fss()  # harmless when nothing is patched
        assert (ref.fss, ref.fss_accum) == before
    finally:
        register.unpatch_fss()
        register.unregister_fft()
