"""The hard planes and the oracle of tests/helpers/moments.py on their own (no GPU): the planes are as hard as their
names promise, the reference's float64 np.mean / np.std stay far inside the project's bar on them (so every bar the
GPU tests compute live is a tight one), and the longdouble oracle agrees with exact rationals."""

import numpy as np
import pytest

from helpers import moments as hard

ALL_CASES = hard.shape_cases() + hard.edge_cases()


def _or_skip(fn, *args):
    try:
        return fn(*args)
    except hard.OracleUnavailable as why:
        pytest.skip(str(why))


@pytest.mark.parametrize("shape", hard.SHAPES, ids=lambda s: "%dx%d" % s)
def test_every_plane_has_the_first_pixel_distance_its_name_promises(shape):
    seen = {}
    for family in hard.FAMILIES:
        seen[family] = _or_skip(hard.first_pixel_distance, hard.plane(family, shape))
    print("\n%s d = |x[0] - mean| / std: %s" % (shape, seen))
    for family in hard.HARD_FAMILIES:
        assert seen[family] >= 50.0, (family, seen[family])
    assert seen["benign"] <= 5.0, seen["benign"]
    for family in hard.SPIKE_ROLLS[1:]:  # the spike anywhere else: the first pixel is an ordinary one
        assert seen[family] <= 5.0, (family, seen[family])
    x = hard.plane("corner_cell_band", shape)
    assert np.argmax(np.abs(x)) == 0  # the band's peak is the first pixel


def test_the_large_edge_planes_are_hard_too():
    for family, shape in hard.edge_cases():
        if family == "spike_first" and shape[0] >= hard.GRID_STRIDE - 1:
            assert _or_skip(hard.first_pixel_distance, hard.plane(family, shape)) >= 50.0


def test_the_spike_rolls_are_one_plane():
    for shape in hard.SHAPES:
        first = hard.plane("spike_first", shape).reshape(-1)
        assert first[0] == hard.SPIKE
        for family in hard.SPIKE_ROLLS:
            x = hard.plane(family, shape).reshape(-1)
            at = hard._roll_of(family, x.size)
            assert x[at] == hard.SPIKE and np.array_equal(np.roll(x, -at), first)


@pytest.mark.parametrize("family,shape", ALL_CASES, ids=[hard.case_id(*c) for c in ALL_CASES])
def test_the_reference_alone_stays_inside_the_cap(family, shape):
    """np.mean / np.std against the oracle: the std never deviates by more than the project's recorded bar (5 x
    deviation_moments, relative to the plane's std) - so no live std bar exceeds it.  The mean is held the same way but
    for the offset family, whose mean carries 2^-53 |mean| / std of inherent rounding."""
    x = hard.plane(family, shape)
    want = _or_skip(hard.case_oracle, family, shape)
    (bar_mean, bar_std), (dev_mean, dev_std) = hard.bars(x, want)
    cap = hard.cap()
    print("\n%s: np.mean %.3g, np.std %.3g of the std; bars %.3g %.3g; cap %.3g" % (hard.case_id(family, shape), dev_mean, dev_std,
                                                                                  bar_mean, bar_std, cap))
    assert 8.0e-14 < cap < 8.2e-14
    assert dev_std <= cap and hard.FLOOR <= bar_std <= cap, (dev_std, bar_std, cap)
    if family == "offset_first_outlier":
        inherent = hard.U * abs(want[0]) / want[1]
        assert dev_mean <= 4.0 * inherent, (dev_mean, inherent)
    else:
        assert dev_mean <= cap and bar_mean <= cap, (dev_mean, bar_mean, cap)


def test_constant_planes_leave_numpy_a_std_of_rounding_order():
    """why the GPU test of the constant planes does not demand an exact zero: NumPy's own pairwise mean can miss c"""
    for shape in hard.SHAPES:
        for c in hard.CONSTANTS:
            x = hard.constant_plane(c, shape)
            assert abs(float(np.mean(x)) - c) <= 2.0 * np.spacing(abs(c)) and 0.0 <= float(np.std(x)) <= 4.0 * hard.U * abs(c)


@pytest.mark.skipif(not hard.wide_longdouble(), reason="numpy.longdouble has no 64-bit significand here")
def test_the_longdouble_oracle_agrees_with_exact_rationals():
    """on the planes the rational route takes: the same float64 pair, up to the one double rounding of the longdouble
    route (an ulp)"""
    small = [c for c in ALL_CASES if int(np.prod(c[1])) <= hard.FRACTION_MAX]
    assert len(small) >= len(hard.FAMILIES) + 16
    worst = 0.0
    for family, shape in small:
        x = hard.plane(family, shape)
        wide, exact = hard._oracle_longdouble(x), hard.oracle_fraction(x)
        for a, b in zip(wide, exact):
            worst = max(worst, hard.ulps(a, b))
            assert hard.ulps(a, b) <= 1.0, (family, shape, wide, exact)
    print("\nlongdouble against exact rationals, worst difference: %.1f ulp over %d planes" % (worst, len(small)))
    with pytest.raises(hard.OracleUnavailable):
        hard.oracle_fraction(np.zeros(hard.FRACTION_MAX + 1))


def test_nonfinite_and_constant_builders():
    for kind in hard.NONFINITE:
        x = hard.nonfinite_plane(kind, (67, 129))
        bad = ~np.isfinite(x)
        assert np.count_nonzero(bad) == 1 and bad.reshape(-1)[0 if kind.endswith("first") else -1]
        with np.errstate(invalid="ignore"):
            assert np.isnan(np.std(x))
    assert hard.oracle(hard.constant_plane(-15.0, (64, 64))) == (-15.0, 0.0)
