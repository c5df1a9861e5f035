"""The NumPy restatement of the resident element-wise passes (helpers/elementwise.py), checked on the CPU against the
unmodified reference and NumPy alone.

1. On every case the restatement's zero mask is the reference's; its ``stats`` are NumPy's.
2. The package's own NumPy branch of ``dB_transform`` is the reference bit for bit, metadata and their types included,
   for every threshold type.
3. The reference's own deviation from the float64 values is reproducible: it is what tests/golden/elementwise_bars.json
   holds, and the device's bar is 5 x that.
4. The rule that leaves an inverse decision open next to the threshold stays under its cap for the reference itself.
"""

import warnings

import numpy as np
import pytest

from helpers import elementwise as ew


@pytest.fixture(scope="module")
def ref_db(ref_pysteps):
    from pysteps.utils.transformation import dB_transform

    return dB_transform


def _quiet(fn, *args, **kwargs):
    # log10 of 0 or of a negative value, 10^x beyond FLT_MAX: the reference warns, the results are what is compared
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*args, **kwargs)


def _call(fn, case):
    return _quiet(fn, case.R.copy(), case.metadata(), threshold=case.threshold, zerovalue=case.zerovalue, inverse=case.inverse)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _same_metadata(a, b):
    if a.keys() != b.keys():
        return False
    for k in a:
        if type(a[k]) is not type(b[k]):
            return False
        if not (a[k] == b[k] or (a[k] != a[k] and b[k] != b[k])):
            return False
    return True


def test_cases_cover_what_they_claim():
    cs = ew.cases()
    names = [c.name for c in cs]
    assert len(set(names)) == len(names)
    sizes = {c.R.size for c in cs}
    assert set(ew.SIZES) | {ew.STATS_LOOP, ew.GRID_STRIDE, 37 * 53} <= sizes
    assert ew.STATS_LOOP > 1024 * 256 and ew.GRID_STRIDE > 256 * 8 * 256 * 4 and ew.GRID_STRIDE % 4
    assert (37 * 53 * 4) % 16 == 4 and (2 * 37 * 53 * 4) % 16 == 8
    kinds = {type(c.threshold) for c in cs}
    assert {float, int, np.float32, np.float64} <= kinds
    # the metadata of a forward transform holds a NumPy scalar: the ordinary inverse is decided in its type
    assert type(ew.forward_threshold_db(0.1)) is np.float64 and type(ew.forward_threshold_db(np.float32(0.1))) is np.float32
    q = ew.quantised(0.7)
    assert q[4] == np.float32(0.7) and q[3] < q[4] < q[5]
    # the four thresholds of the defect: float32(thr) is dry against the float64 scalar and wet against the float
    for thr in (0.7, 0.03, 0.08, 0.16):
        assert ew.less_than(np.array([thr], np.float32), np.float64(thr))[0]
        assert not ew.less_than(np.array([thr], np.float32), thr)[0]
        assert ew.compared_with(thr) == float(np.float32(thr)) and ew.compared_with(np.float64(thr)) == thr


@pytest.mark.parametrize("case", ew.cases(), ids=lambda c: c.name)
def test_zero_mask_is_the_references(ref_db, case):
    got, _ = _call(ref_db, case)
    assert got.dtype == np.float32
    zeroed = got == np.float32(case.zerovalue)
    if not case.inverse:
        exp = ew.expectation(case)
        assert np.array_equal(zeroed, exp.zeros)
        # what is not zeroed is the float32 evaluation of the float64 value: NaN stays NaN, infinities stay
        dev, wrong = ew.deviation(got, exp.value, ~exp.zeros)
        assert wrong == 0 and dev <= 1.001 * ew.load_bars()["forward"]["measured"]  # stored to four digits
        return
    own = 1.001 * ew.load_bars()["inverse"]["measured"] * case.bar_scale  # stored to four digits
    exp = ew.expectation(case, bar=own)
    decided = ~exp.near
    assert np.array_equal(zeroed[decided], exp.zeros[decided])
    # next to the threshold either answer is a correct float32 evaluation, but nothing else is
    dev, wrong = ew.deviation(got, exp.value, ~zeroed)
    assert wrong == 0 and dev <= own
    if case.name in ew.ISOLATING_WANT:
        assert got.tolist() == ew.ISOLATING_WANT[case.name]
    if case.continuous:
        assert exp.near_share() <= ew.NEAR_CAP, exp.near_share()


@pytest.mark.parametrize("case", [c for c in ew.cases() if c.inverse and c.continuous], ids=lambda c: c.name)
def test_open_decisions_stay_under_the_cap_at_the_device_bar(ref_db, case):
    """With the window the device is given (5 x the reference's deviation) the reference itself decides every element
    outside it like the float64 value, and the window holds at most 1e-3 of a case."""
    exp = ew.expectation(case, bar=ew.bar("inverse"))
    got, _ = _call(ref_db, case)
    zeroed = got == np.float32(case.zerovalue)
    assert exp.near_share() <= ew.NEAR_CAP, exp.near_share()
    assert np.array_equal(zeroed[~exp.near], exp.zeros[~exp.near])


@pytest.mark.parametrize("case", ew.cases(), ids=lambda c: c.name)
def test_host_branch_is_the_reference_bit_for_bit(ref_db, case):
    from pysteps_amd.utils import dB_transform

    want, wmeta = _call(ref_db, case)
    got, gmeta = _call(dB_transform, case)
    assert _same_bits(got, want)
    assert _same_metadata(gmeta, wmeta), (gmeta, wmeta)


@pytest.mark.parametrize("form,thr", ew.threshold_forms(0.5) + [("none", None)])
def test_host_branch_default_zerovalue_and_metadata_threshold(ref_db, form, thr):
    """zerovalue=None and threshold=None take their values from the metadata, forwards and back."""
    from pysteps_amd.utils import dB_transform

    R = ew.rates(1023, 7)
    meta = {"transform": None, "threshold": np.float32(0.16), "zerovalue": 0.0, "unit": "mm/h"}
    want, wmeta = ref_db(R.copy(), dict(meta), threshold=thr)
    got, gmeta = dB_transform(R.copy(), dict(meta), threshold=thr)
    assert _same_bits(got, want) and _same_metadata(gmeta, wmeta)
    back_w, bw = ref_db(want, wmeta, inverse=True)
    back_g, bg = dB_transform(got, gmeta, inverse=True)
    assert _same_bits(back_g, back_w) and _same_metadata(bg, bw)


@pytest.mark.parametrize("name,a", ew.stats_cases(), ids=[n for n, _ in ew.stats_cases()])
def test_stats_are_numpys(name, a):
    s = ew.stats(a)
    assert s["nonfinite"] == int(np.count_nonzero(~np.isfinite(a)))
    assert s["neg_inf"] == int(np.count_nonzero(np.isneginf(a))) and s["pos_inf"] == int(np.count_nonzero(np.isposinf(a)))
    fin = np.where(np.isfinite(a), a, np.nan)
    if a.size == 0:
        assert np.isnan(s["nanmin"]) and s["min_finite"] == np.inf and s["max_finite"] == -np.inf
        return
    want_nanmin = _quiet(np.nanmin, a)
    assert s["nanmin"] == want_nanmin or (np.isnan(s["nanmin"]) and np.isnan(want_nanmin))
    if np.isfinite(a).any():
        assert s["min_finite"] == np.nanmin(fin) and s["max_finite"] == np.nanmax(fin)
    else:
        assert s["min_finite"] == np.inf and s["max_finite"] == -np.inf


def test_convert_pattern_holds_what_it_claims():
    with np.errstate(over="ignore"):
        w = ew.wide_pattern().astype(np.float32)
    e = np.float32(2.0 ** -22)
    assert w[0] == 1 and w[1] == 1 + e and w[2] == 1 + e and w[3] == 1 + e / 2 and w[4] == 1
    assert w[9] == np.float32(ew.FLT_MAX) and w[10] == np.float32(ew.FLT_MAX) and np.all(np.isinf(w[11:16]))
    assert 0 < w[16] < np.float32(ew.FLT_MIN) and w[20] == 0 and w[21] == np.float32(2.0 ** -148) and w[22] == w[21]


def test_bars_are_reproducible(ref_db):
    """Recomputing the reference's deviation gives the values in the JSON, to the four digits it stores; the device's bar
    is 5 x that."""
    rec = ew.load_bars()
    assert rec["bar_factor"] == ew.BAR_FACTOR == 5.0
    for direction, (dev, where) in ew.measure(ref_db).items():
        assert ew.stored(dev) == rec[direction]["measured"], (direction, dev, where)
        assert where == rec[direction]["worst_case"]
        assert rec[direction]["bar"] == pytest.approx(ew.BAR_FACTOR * rec[direction]["measured"], rel=1e-12)
        assert ew.bar(direction) == rec[direction]["bar"]
        # a float32 evaluation cannot be closer than its own rounding; a bar of hundreds of spacings would hold nothing
        assert 0.5 <= rec[direction]["measured"] < 20.0


def test_the_check_has_teeth():
    """A result one bar and a spacing off fails; a threshold compared in the wrong type flips the level that sits on it."""
    R = ew.rates(4099, 11)
    exp = ew.db_forward(R, 0.1, ew.FORWARD_ZERO)
    good = exp.value.astype(np.float32)
    assert ew.deviation(good, exp.value, ~exp.zeros)[0] <= 0.5
    bad = good.copy()
    k = int(np.flatnonzero(~exp.zeros)[17])
    bad[k] += np.float32((ew.bar("forward") + 1.0) * ew.spacing32(exp.value[k]))
    assert ew.deviation(bad, exp.value, ~exp.zeros)[0] > ew.bar("forward")
    q = ew.quantised(0.7)
    assert np.count_nonzero(ew.db_forward(q, 0.7, 0).zeros != ew.db_forward(q, np.float64(0.7), 0).zeros) == 1
