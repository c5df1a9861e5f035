"""Temporal autocorrelation and the AR estimate on the device (csrc/autocorr.hip, pysteps_amd/timeseries) against the
goldens of the unmodified reference and the exact restatement of tests/helpers/autocorr.py.

Yardsticks.  Global coefficients: 5 x the reference's own deviation from the exact coefficients (integer sums,
longdouble finish), measured by tools/make_golden_autocorr.py - ``deviation_spatial`` 1.33e-15, ``deviation_spectral``
5.55e-16, absolute; AR parameters 5 x ``deviation_phi``.  Sums: every double-double sum against the exact integer sum,
within 4 x 2^-106 per addition on a value's way (a sloppy double-double addition is good to 3 x 2^-106 of the
magnitudes it adds; the products are exact) of the sum of the terms' magnitudes; counts without tolerance.  Rows of a
cascade against per-level calls, a second run, a level viewed out of a larger stack, an aligned against a misaligned
stack, and the moving-window planes against the goldens: bit for bit.
"""

import math
import os
import warnings
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN, nan_mismatch, rel_l2
from helpers import autocorr as restated

pytestmark = pytest.mark.gpu

PATH = os.path.join(GOLDEN, "autocorr_reference.npz")
SPATIAL = restated.spatial_cases()
seen_spatial, seen_spectral = [0.0], [0.0]


@pytest.fixture(scope="module")
def golden():
    return np.load(PATH)


@pytest.fixture(scope="module")
def mods():
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.timeseries import autoregression, correlation

    return correlation, autoregression, DeviceArray


def _device_mask(DeviceArray, mask):
    return None if mask is None else DeviceArray.from_host(mask.view(np.uint8))


@pytest.mark.parametrize("case", SPATIAL, ids=[c[0] for c in SPATIAL])
def test_spatial_coefficients(golden, mods, case):
    correlation, _, DeviceArray = mods
    name, shape, L, T, d, dtype, kind, variant = case
    x, mask = restated.cascade(shape, L, T, dtype, variant), restated.mask_of(kind, shape)
    resident = SPATIAL.index(case) % 2 == 0
    if resident:
        stack, dmask = DeviceArray.from_host(x), _device_mask(DeviceArray, mask)
        level = stack.view
    else:
        stack, dmask = x, mask
        level = lambda l: x[l]  # noqa: E731
    got = correlation.cascade_autocorrelation(stack, mask=dmask, d=d)
    assert got.shape == (L, T - d - 1) and got.dtype == np.float64
    vs_exact = restated.max_abs_dev(got, golden[name + "__exact"])
    vs_ref = restated.max_abs_dev(got, golden[name + "__ref"])
    seen_spatial[0] = max(seen_spatial[0], vs_exact)
    print("\n%s: %.3g from the exact coefficients, %.3g from the reference's (bar %.3g)"
          % (name, vs_exact, vs_ref, 5 * float(golden["deviation_spatial"])))
    assert vs_exact <= 5 * float(golden["deviation_spatial"]) and vs_ref <= 5 * float(golden["deviation_spatial"])
    assert np.array_equal(got, correlation.cascade_autocorrelation(stack, mask=dmask, d=d), equal_nan=True)  # a second run
    for l in range(L):  # resident: a level viewed out of the stack, every second one 8 bytes off for an odd pixel count
        row = correlation.temporal_autocorrelation(level(l), d=d, mask=dmask)
        assert isinstance(row, list) and all(type(v) is float for v in row)
        assert np.array_equal(np.array(row, dtype=np.float64), got[l], equal_nan=True), (name, l)
    if kind in ("one", "empty") or (variant == "constant" and d == 0):
        assert np.isnan(got).all()
    if variant == "identical" and d == 0:
        assert np.array_equal(got[:, 0], np.ones(L))


def test_measured_spatial_deviation_is_reported(golden):
    print("\nlargest device deviation from the exact spatial coefficients: %.3g (the reference's: %.3g)"
          % (seen_spatial[0], float(golden["deviation_spatial"])))
    assert seen_spatial[0] <= 5 * float(golden["deviation_spatial"])


SUM_CASES = [((5, 7), 3, 4, 0, "float64", "none"), ((61, 67), 3, 3, 0, "float64", "sparse"), ((61, 67), 3, 4, 1, "float64", "all"),
             ((61, 67), 8, 3, 1, "float32", "sparse"), ((257, 263), 1, 4, 0, "float64", "sparse"), ((257, 263), 3, 2, 0, "float32", "none"),
             ((257, 263), 1, 10, 1, "float64", "sparse")]  # the last: eight lags, the wide kernel


@pytest.mark.parametrize("case", SUM_CASES, ids=["%dx%d_L%d_T%d_d%d_%s_%s" % (c[0] + c[1:]) for c in SUM_CASES])
def test_sums_against_exact_integers(mods, case):
    correlation, _, DeviceArray = mods
    shape, L, T, d, dtype, kind = case
    x, mask = restated.cascade(shape, L, T, dtype), restated.mask_of(kind, shape)
    npix = shape[0] * shape[1]
    sums, count, bad = correlation.spatial_sums(DeviceArray.from_host(x), L, T, npix, _device_mask(DeviceArray, mask), d)
    assert count == (npix if mask is None else int(mask.sum())) and not bad.any() and bad.shape == (L,)
    assert sums.shape == (L, 2 + 3 * (T - d - 1), 2)
    blocks = min(512, -(-((npix + 1) // 2) // 256))
    adds = 2 * -(-((npix + 1) // 2) // (blocks * 256)) + 6 + 3 + -(-blocks // 256) + 6 + 3
    bar = adds * 4 * Fraction(1, 1 << 106)
    worst = 0.0
    for l in range(L):
        n, rows = restated.exact_sums(x[l], d, mask, restated._GRID[dtype])
        scale = restated.exact_abs_sums(x[l], d, mask, restated._GRID[dtype])
        assert n == count
        for s, (want, mag) in enumerate(zip(rows, scale)):
            err = abs(restated.dd_value(sums[l, s]) - want)
            worst = max(worst, float(err / mag * (1 << 106)))
            assert err <= bar * mag, (l, s, float(err / mag), float(bar))
    print("\n%s: worst sum %.2f units of 2^-106 of the terms' magnitudes (bar %d: %d additions)" % (case, worst, 4 * adds, adds))


def test_alignment_and_position_do_not_change_the_bits(mods):
    """An even pixel count: the aligned stack takes the two-element loads, the same stack 8 bytes (float32: 4) further
    the element-wise path; a stack inside a larger one; all the same bits."""
    correlation, _, DeviceArray = mods
    for dtype in ("float64", "float32"):
        x = restated.cascade((16, 18), 3, 3, dtype)
        mask = restated.mask_of("sparse", (16, 18))
        dmask = _device_mask(DeviceArray, mask)
        want = correlation.cascade_autocorrelation(DeviceArray.from_host(x), mask=dmask, d=1)
        padded = np.zeros(x.size + 4, dtype=x.dtype)
        for shift in (1, 2, 3):
            padded[shift:shift + x.size] = x.reshape(-1)
            big = DeviceArray.from_host(padded)
            moved = DeviceArray(x.shape, x.dtype, ptr=big.ptr + shift * x.dtype.itemsize, owner=big)
            assert np.array_equal(correlation.cascade_autocorrelation(moved, mask=dmask, d=1), want), (dtype, shift)
        assert np.array_equal(correlation.cascade_autocorrelation(x, mask=mask, d=1), want)  # host input
        assert restated.max_abs_dev(want, [restated.exact_gamma(x[l], 1, mask, dtype) for l in range(3)]) < 1e-15


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_a_nonfinite_value_outside_the_mask_raises(mods, value):
    correlation, _, DeviceArray = mods
    x = restated.cascade((61, 67), 3, 3, "float64")
    mask = restated.mask_of("sparse", (61, 67))
    outside = np.flatnonzero(~mask.reshape(-1))[5]
    x[2, 0].reshape(-1)[outside] = value  # the oldest plane of the last level: differencing would not hide it either
    for d in (0, 1):
        with pytest.raises(ValueError, match="^x contains non-finite values$"):
            correlation.cascade_autocorrelation(DeviceArray.from_host(x), mask=_device_mask(DeviceArray, mask), d=d)
        with pytest.raises(ValueError, match="^x contains non-finite values$"):
            correlation.temporal_autocorrelation(x[2], mask=mask, d=d)
        assert np.isfinite(correlation.temporal_autocorrelation(x[1], mask=mask, d=d)).all()
    _, _, bad = correlation.spatial_sums(DeviceArray.from_host(x), 3, 3, 61 * 67, _device_mask(DeviceArray, mask), 0)
    assert [int(v) for v in bad] == [0, 0, 1]
    with pytest.raises(ValueError, match="^x contains non-finite values$"):
        correlation.temporal_autocorrelation(x[2], mask=mask, window_radius=4)


def test_declined_resident_input_raises(mods):
    correlation, _, DeviceArray = mods
    with pytest.raises(NotImplementedError, match="10 lags"):
        correlation.temporal_autocorrelation(DeviceArray((11, 5, 7), np.float64).fill_bytes(0))
    with pytest.raises(NotImplementedError, match="dtype uint8"):
        correlation.temporal_autocorrelation(DeviceArray((3, 5, 7), np.uint8).fill_bytes(0))


@pytest.mark.parametrize("case", restated.spectral_cases(), ids=[c[0] for c in restated.spectral_cases()])
def test_spectral_coefficients(golden, mods, case):
    correlation, _, DeviceArray = mods
    name, shape, L, T, d, full = case
    x = restated.spectral_cascade(golden["spec_%dx%d" % shape], L, T, full, shape[1])
    resident = DeviceArray.from_host(x)
    got = correlation.cascade_autocorrelation(resident, d=d, domain="spectral", x_shape=shape, use_full_fft=full)
    assert got.shape == (L, T - d - 1)
    vs_exact = restated.max_abs_dev(got, golden[name + "__exact"])
    vs_ref = restated.max_abs_dev(got, golden[name + "__ref"])
    vs_fields = restated.max_abs_dev(got, golden[name + "__spatial"])
    seen_spectral[0] = max(seen_spectral[0], vs_exact)
    print("\n%s: %.3g from the exact coefficients, %.3g from the reference's (bar %.3g), %.3g from the fields' (bar %.3g)"
          % (name, vs_exact, vs_ref, 5 * float(golden["deviation_spectral"]), vs_fields, restated.parseval_bar(shape, 1)))
    assert vs_exact <= 5 * float(golden["deviation_spectral"]) and vs_ref <= 5 * float(golden["deviation_spectral"])
    assert vs_fields <= restated.parseval_bar(shape, 1)
    assert np.array_equal(got, correlation.cascade_autocorrelation(x, d=d, domain="spectral", x_shape=shape, use_full_fft=full))
    for l in range(L):
        for series in (resident.view(l), x[l]):
            row = correlation.temporal_autocorrelation(series, d=d, domain="spectral", x_shape=shape, use_full_fft=full)
            assert np.array_equal(np.array(row), got[l]), (name, l)
    bad = x.copy()
    bad[L - 1, 0, 3, 2] = complex(0.0, np.inf)
    with pytest.raises(ValueError, match="^x contains non-finite values$"):
        correlation.cascade_autocorrelation(bad, d=d, domain="spectral", x_shape=shape, use_full_fft=full)


def test_measured_spectral_deviation_is_reported(golden):
    print("\nlargest device deviation from the exact spectral coefficients: %.3g (the reference's: %.3g)"
          % (seen_spectral[0], float(golden["deviation_spectral"])))
    assert seen_spectral[0] <= 5 * float(golden["deviation_spectral"])


@pytest.mark.parametrize("case", restated.window_cases(), ids=[c[0] for c in restated.window_cases()])
def test_moving_window_planes_equal_the_references(golden, mods, case):
    correlation, _, DeviceArray = mods
    name, T, d, sigma, masked = case
    x = np.ascontiguousarray(golden["series_%dx%d" % restated.WINDOW_SHAPE][:T])
    mask = restated.window_mask(restated.WINDOW_SHAPE) if masked else None
    want = golden[name + "__ref"]
    got = correlation.temporal_autocorrelation(x, d=d, mask=mask, window_radius=sigma)
    assert isinstance(got, list) and len(got) == T - d - 1 and all(isinstance(p, np.ndarray) for p in got)
    assert np.array_equal(np.array(got), want, equal_nan=True)
    uniform = correlation.temporal_autocorrelation(x, d=d, mask=mask, window="uniform", window_radius=sigma)
    assert np.array_equal(np.array(uniform), want, equal_nan=True)  # the reference never passes window= on
    planes = correlation.temporal_autocorrelation(DeviceArray.from_host(x), d=d, mask=_device_mask(DeviceArray, mask), window_radius=sigma)
    assert all(isinstance(p, DeviceArray) and p.shape == restated.WINDOW_SHAPE for p in planes)
    assert np.array_equal(np.array([p.to_host() for p in planes]), want, equal_nan=True)
    if masked:
        assert np.isnan(np.array(got)[:, :6, :8]).all()  # around the two-pixel island: fewer than three values
    assert np.isnan(want).all() == (sigma == 1.5)


def test_cascade_ar_params_is_the_host_chain_on_the_device_coefficients(golden, mods):
    correlation, ar, DeviceArray = mods
    checked, worst = 0, 0.0
    for name, shape, L, T, d, dtype, kind, variant in SPATIAL:
        if name + "__phi" not in golden.files:
            continue
        x, mask = restated.cascade(shape, L, T, dtype, variant), restated.mask_of(kind, shape)
        stack, dmask = DeviceArray.from_host(x), _device_mask(DeviceArray, mask)
        gamma, phi = ar.cascade_ar_params(stack, mask=dmask)
        raw = correlation.cascade_autocorrelation(stack, mask=dmask)
        for l in range(L):
            g = raw[l].copy()
            if g.size == 2:
                g[1] = ar.adjust_lag2_corrcoef2(g[0], g[1])
            assert np.array_equal(gamma[l], g) and np.array_equal(phi[l], ar.estimate_ar_params_yw(g))
        worst = max(worst, float(np.max(np.abs(phi - golden[name + "__phi"]))))
        assert np.max(np.abs(phi - golden[name + "__phi"])) <= 5 * float(golden["deviation_phi"]), name
        checked += 1
    assert checked >= 30
    print("\nAR parameters of %d cascades: %.3g from the reference's (bar %.3g)" % (checked, worst, 5 * float(golden["deviation_phi"])))


def test_sprog_with_the_swapped_autocorrelation(ref_pysteps, monkeypatch):
    """The real nowcasts.sprog.forecast of the reference, 128 x 128, 3 lead times, 6 levels: with
    register(correlation=True) its autocorrelation comes from the device, and the forecast stays within the caller bar
    of docs/history.md (1e-4 relative L2, equal NaN masks) of the stock route."""
    from pysteps import nowcasts
    from pysteps.timeseries import correlation as ref

    from pysteps_amd import register
    from pysteps_amd.timeseries import correlation
    from tools import synth

    frames = synth.steps_frames(128, 128, 3)
    V = synth.true_velocity(128, 128).astype(np.float64)
    sprog = nowcasts.get_method("sprog")
    kw = dict(n_cascade_levels=6, precip_thr=-10.0)
    calls = []
    sums = correlation.spatial_sums
    monkeypatch.setattr(correlation, "spatial_sums", lambda *a: calls.append(a[1:4]) or sums(*a))
    try:
        register.register()
        want = sprog(frames, V, 3, **kw)
        assert not calls
        assert register.register(correlation=True)[-1] == "correlation:temporal_autocorrelation"
        assert ref.temporal_autocorrelation is correlation.temporal_autocorrelation
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            got = sprog(frames, V, 3, **kw)
        assert not [w for w in caught if "pysteps_amd" in str(w.message)]  # nothing is declined
    finally:
        register.unpatch_correlation()
        register.unregister_fft()
    assert calls == [(1, 3, 128 * 128)] * 6  # one call per cascade level, on the device
    assert got.shape == want.shape == (3, 128, 128) and nan_mismatch(got, want) == 0
    rel = rel_l2(got, want)
    print("\nsprog 128 x 128: relative L2 %.3g between the device and the stock autocorrelation" % rel)
    assert rel < 1e-4 and math.isfinite(rel)
