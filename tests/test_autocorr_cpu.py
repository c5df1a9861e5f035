"""Temporal autocorrelation and the AR estimate, host side (no GPU): the restatements of tests/helpers/autocorr.py
against the goldens of the unmodified reference, the host restatements of the AR estimate, the argument checks, the
Python layer's exact finish with integer sums standing in for the kernels, and the registration.

Yardsticks.  Global coefficients: the reference's own deviation from the exact coefficients (integer sums, longdouble
finish), measured by tools/make_golden_autocorr.py over every case - 1.33e-15 spatial, 5.55e-16 spectral, absolute -
and 5 x that for anything that sums in another order.  Moving-window planes and the AR estimate: no tolerance.
"""

import json
import os
import warnings

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import autocorr as restated

PATH = os.path.join(GOLDEN, "autocorr_reference.npz")
SPATIAL = restated.spatial_cases()
SMALL = [c for c in SPATIAL if c[1] != (257, 263)]


@pytest.fixture(scope="module")
def golden():
    return np.load(PATH)


def test_golden_covers_the_required_cases(golden):
    assert [str(n) for n in golden["spatial_cases"]] == [c[0] for c in SPATIAL]
    assert [str(n) for n in golden["spectral_cases"]] == [c[0] for c in restated.spectral_cases()]
    assert [str(n) for n in golden["window_cases"]] == [c[0] for c in restated.window_cases()]
    assert {c[1] for c in SPATIAL} == {(5, 7), (61, 67), (257, 263)} and {c[2] for c in SPATIAL} == {1, 3, 8}
    assert {c[3] for c in SPATIAL} == {2, 3, 4} and {c[4] for c in SPATIAL} == {0, 1} and {c[5] for c in SPATIAL} == {"float32", "float64"}
    assert {c[6] for c in SPATIAL} == set(restated.MASKS) and {c[7] for c in SPATIAL} == set(restated.VARIANTS)
    for shape in restated.SHAPES:  # every shape under every number of levels, frames, d and dtype
        assert len({c[2:6] for c in SPATIAL if c[1] == shape}) >= 36
    assert 0.0 < float(golden["deviation_spatial"]) < 1e-14 and 0.0 < float(golden["deviation_spectral"]) < 1e-14
    assert abs(float(golden["deviation_spatial"]) - 1.33e-15) < 1e-17 and abs(float(golden["deviation_spectral"]) - 5.55e-16) < 1e-18
    assert float(golden["deviation_spatial"]) < float(golden["deviation_phi"]) < 1e-12
    assert os.path.getsize(PATH) < 512 * 1024


def test_generator_reproduces_the_stored_inputs(golden):
    for shape in restated.STORED_SHAPES:
        assert np.array_equal(golden["series_%dx%d" % shape], restated.cascade(shape, 1, 4, "float64")[0])
    x32, x64 = restated.cascade((61, 67), 3, 4, "float32"), restated.cascade((61, 67), 3, 4, "float64")
    assert x32.dtype == np.float32 and x64.dtype == np.float64
    assert np.abs(x64).max() < 128 and np.array_equal(x64 * 2.0**45, np.round(x64 * 2.0**45))
    assert np.abs(x32).max() < 32 and np.array_equal(x32.astype(np.float64) * 2.0**18, np.round(x32.astype(np.float64) * 2.0**18))
    bits = np.abs(x64 * 2.0**45).astype(np.int64)
    assert (bits & 0xFFFFF).any() and (bits >> 45).any()  # low and high bits in use: a product needs more than 53
    assert restated.mask_of("two", (61, 67)).sum() == 2 and restated.mask_of("one", (61, 67)).sum() == 1
    assert not restated.mask_of("empty", (5, 7)).any() and 0.03 < restated.mask_of("sparse", (257, 263)).mean() < 0.07


@pytest.mark.parametrize("case", SPATIAL, ids=[c[0] for c in SPATIAL])
def test_restatement_reproduces_the_spatial_goldens(golden, case):
    name, shape, L, T, d, dtype, kind, variant = case
    x, mask = restated.cascade(shape, L, T, dtype, variant), restated.mask_of(kind, shape)
    got = np.array([restated.reference_float64(x[l], d=d, mask=mask) for l in range(L)], dtype=np.float64).reshape(L, T - d - 1)
    assert restated.max_abs_dev(got, golden[name + "__ref"]) <= float(golden["deviation_spatial"])
    assert restated.max_abs_dev(golden[name + "__exact"], golden[name + "__ref"]) <= float(golden["deviation_spatial"])
    if kind in ("one", "empty") or variant == "constant" and d == 0:
        assert np.isnan(golden[name + "__ref"]).all() and np.isnan(golden[name + "__exact"]).all()
    if variant == "identical" and d == 0:
        assert np.array_equal(golden[name + "__exact"][:, 0], np.ones(L))


@pytest.mark.parametrize("case", restated.spectral_cases(), ids=[c[0] for c in restated.spectral_cases()])
def test_restatement_reproduces_the_spectral_goldens(golden, case):
    name, shape, L, T, d, full = case
    x = restated.spectral_cascade(golden["spec_%dx%d" % shape], L, T, full, shape[1])
    got = np.array([restated.reference_float64(x[l], d=d, domain="spectral", x_shape=shape, use_full_fft=full) for l in range(L)])
    assert restated.max_abs_dev(got.reshape(L, -1), golden[name + "__ref"]) <= float(golden["deviation_spectral"])
    # Parseval: the coefficient of the spectra is the coefficient of the fields, up to the transform's rounding
    assert restated.max_abs_dev(golden[name + "__exact"], golden[name + "__spatial"]) <= restated.parseval_bar(shape, 1)
    if full:  # the completed spectrum is the transform of a real field
        fields = restated.cascade(shape, 1, 4, "float64")[0]
        assert np.allclose(x[0, 0], np.fft.fft2(fields[0]), rtol=0, atol=1e-9)


@pytest.mark.parametrize("case", restated.window_cases(), ids=[c[0] for c in restated.window_cases()])
def test_restatement_reproduces_the_window_goldens(golden, case):
    name, T, d, sigma, masked = case
    x = golden["series_%dx%d" % restated.WINDOW_SHAPE][:T]
    mask = restated.window_mask(restated.WINDOW_SHAPE) if masked else np.ones(restated.WINDOW_SHAPE, dtype=bool)
    got = np.array(restated.reference_float64(x, d=d, mask=mask, window_radius=sigma))
    assert got.shape == (T - d - 1,) + restated.WINDOW_SHAPE and np.array_equal(got, golden[name + "__ref"], equal_nan=True)
    assert np.isnan(got).all() == (sigma == 1.5)  # n <= sigma**2 = 2.25 fails the reference's n >= 3 everywhere
    if masked:
        assert np.isnan(got[:, :6, :8]).all()  # around the two-pixel island


def test_ar_restatements_equal_the_references_outputs(golden):
    from pysteps_amd.timeseries import autoregression as ar

    gammas = np.array(restated.AR_GAMMAS, dtype=np.float64)
    assert np.array_equal(golden["ar_adjust1"], [ar.adjust_lag2_corrcoef1(g[0], g[1]) for g in gammas])
    assert np.array_equal(golden["ar_adjust2"], [ar.adjust_lag2_corrcoef2(g[0], g[1]) for g in gammas])
    messages = json.loads(str(golden["messages"]))
    seen_raise = False
    for p in (1, 2, 3):
        for d in (0, 1):
            want, raised = golden["ar_yw_p%d_d%d" % (p, d)], golden["ar_yw_raised_p%d_d%d" % (p, d)]
            for g, row, bad in zip(gammas, want, raised):
                if bad:
                    seen_raise = True
                    with pytest.raises(RuntimeError) as exc:
                        ar.estimate_ar_params_yw(g[:p], d=d)
                    assert ["RuntimeError", str(exc.value)] == messages["nonstationary"]
                else:
                    got = ar.estimate_ar_params_yw(g[:p], d=d)
                    assert got.shape == (p + d + 1,) and np.array_equal(got, row)
        unchecked = np.array([ar.estimate_ar_params_yw(g[:p], check_stationarity=False) for g in gammas])
        assert np.array_equal(unchecked, golden["ar_yw_unchecked_p%d" % p])
        assert [ar.test_ar_stationarity(row[:p]) for row in unchecked] == [bool(v) for v in golden["ar_stationary_p%d" % p]]
    assert seen_raise
    with pytest.raises(RuntimeError) as exc:
        ar.estimate_ar_params_yw(np.array(restated.AR_NONSTATIONARY))
    assert ["RuntimeError", str(exc.value)] == messages["nonstationary"]
    with pytest.raises(ValueError) as exc:
        ar.estimate_ar_params_yw(gammas[0], d=2)
    assert ["ValueError", str(exc.value)] == messages["yw_d"]


def test_argument_checks_raise_the_references_messages_without_a_device(golden, monkeypatch):
    from pysteps_amd import _lib
    from pysteps_amd.timeseries import correlation

    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the checks must not touch the device"))
    messages = json.loads(str(golden["messages"]))
    calls = {"dimension": (ValueError, lambda: correlation.temporal_autocorrelation(np.zeros(5))),
             "spectral": (NotImplementedError, lambda: correlation.temporal_autocorrelation(np.zeros((3, 2, 4, 4), dtype=complex),
                                                                                            domain="spectral")),
             "mask": (ValueError, lambda: correlation.temporal_autocorrelation(np.zeros((3, 4, 5)), mask=np.ones((4, 4), dtype=bool)))}
    for key, (kind, call) in calls.items():
        with pytest.raises(kind) as exc:
            call()
        assert [kind.__name__, str(exc.value)] == messages[key], key
    assert messages["nonfinite"] == ["ValueError", "x contains non-finite values"]


class _Host:
    """What the layer needs of an uploaded array, on the host."""

    def __init__(self, a):
        self.a, self.shape, self.dtype = a, a.shape, a.dtype


@pytest.fixture
def host_sums(monkeypatch):
    """The Python layer with the helpers' integer sums in place of ``psh_autocorr_sums_dev``: each exact sum split into
    a double-double pair."""
    from pysteps_amd.timeseries import correlation

    def pair(frac):
        hi = float(frac)
        return [hi, float(frac - restated.Fraction(hi))]

    def spatial_sums(stack, L, T, npix, mask, d):
        x = stack.a.reshape(L, T, npix)
        grid = restated._GRID[str(x.dtype)]
        flat_mask = None if mask is None else mask.a.reshape(-1).astype(bool)
        rows = [restated.exact_sums(x[l], d, flat_mask, grid) for l in range(L)]
        sums = np.array([[pair(v) for v in r[1]] for r in rows], dtype=np.float64).reshape(L, 2 + 3 * (T - d - 1), 2)
        return sums, rows[0][0], np.array([np.count_nonzero(~np.isfinite(x[l])) for l in range(L)], dtype=np.uint64)

    monkeypatch.setattr(correlation, "spatial_sums", spatial_sums)
    monkeypatch.setattr(correlation, "_upload", lambda a: _Host(np.ascontiguousarray(a)))
    monkeypatch.setattr(correlation, "_upload_mask", lambda m: None if m is None else _Host(np.ascontiguousarray(m).view(np.uint8)))
    return correlation


@pytest.mark.parametrize("case", SMALL, ids=[c[0] for c in SMALL])
def test_python_layer_finishes_exact_sums_to_the_exact_coefficients(golden, host_sums, case):
    """The rational finish, the NaN rules, the clip and the per-level calls, with exact sums: the correctly rounded
    coefficient, so the longdouble restatement's own rounding (2^-64 relative, then to float64) is all that may differ."""
    name, shape, L, T, d, dtype, kind, variant = case
    x, mask = restated.cascade(shape, L, T, dtype, variant), restated.mask_of(kind, shape)
    got = host_sums.cascade_autocorrelation(x, mask=mask, d=d)
    assert got.shape == (L, T - d - 1) and got.dtype == np.float64
    assert restated.max_abs_dev(got, golden[name + "__exact"]) <= 2.0**-52
    assert restated.max_abs_dev(got, golden[name + "__ref"]) <= 5 * float(golden["deviation_spatial"])
    for l in range(L):
        row = host_sums.temporal_autocorrelation(x[l], d=d, mask=mask)
        assert isinstance(row, list) and all(type(v) is float for v in row)
        assert np.array_equal(np.array(row, dtype=np.float64), got[l], equal_nan=True)
    if variant == "identical" and d == 0:
        assert np.array_equal(got[:, 0], np.ones(L))


def test_python_layer_raises_on_a_nonfinite_value_outside_the_mask(host_sums):
    x = restated.cascade((5, 7), 1, 3, "float64")[0].copy()
    mask = restated.mask_of("sparse", (5, 7))
    x[0].reshape(-1)[np.flatnonzero(~mask.reshape(-1))[0]] = np.inf
    with pytest.raises(ValueError, match="^x contains non-finite values$"):
        host_sums.temporal_autocorrelation(x, mask=mask)


def test_cascade_ar_params_is_the_host_chain(golden, host_sums):
    from pysteps_amd.timeseries import autoregression as ar

    checked = 0
    for name, shape, L, T, d, dtype, kind, variant in SMALL:
        if name + "__phi" not in golden.files:
            continue
        x, mask = restated.cascade(shape, L, T, dtype, variant), restated.mask_of(kind, shape)
        gamma, phi = ar.cascade_ar_params(x, mask=mask)
        raw = host_sums.cascade_autocorrelation(x, mask=mask)
        for l in range(L):
            g = raw[l].copy()
            if g.size == 2:
                g[1] = ar.adjust_lag2_corrcoef2(g[0], g[1])
            assert np.array_equal(gamma[l], g) and np.array_equal(phi[l], ar.estimate_ar_params_yw(g))
        assert np.max(np.abs(phi - golden[name + "__phi"])) <= 5 * float(golden["deviation_phi"])
        checked += 1
    assert checked >= 20
    x = restated.cascade((61, 67), 3, 4, "float64")
    gamma, phi = ar.cascade_ar_params(x, ar_order=2)
    assert gamma.shape == (3, 2) and phi.shape == (3, 3)
    with pytest.raises(ValueError, match="ar_order = 4"):
        ar.cascade_ar_params(x, ar_order=4)


def test_decline_reasons_need_no_device():
    from pysteps_amd.timeseries.correlation import _decline_reason

    x = np.zeros((3, 6, 7))
    assert _decline_reason(x, 0, "spatial", None, np.inf) is None and _decline_reason(x.astype(np.float32), 1, "spatial", None, np.inf) is None
    assert "10 lags" in _decline_reason(np.zeros((11, 6, 7)), 0, "spatial", None, np.inf)
    assert _decline_reason(np.zeros((10, 6, 7)), 1, "spatial", None, np.inf) is None  # 8 lags after differencing
    assert "dtype int64" in _decline_reason(x.astype(np.int64), 0, "spatial", None, np.inf)
    assert "complex128" in _decline_reason(x, 0, "spectral", None, np.inf)
    assert _decline_reason(x.astype(complex), 0, "spectral", None, np.inf) is None
    assert "not a boolean" in _decline_reason(x, 0, "spatial", np.ones((6, 7)), np.inf)
    assert _decline_reason(x, 0, "spatial", np.ones((6, 7), dtype=bool), 4) is None
    assert "window_radius=600" in _decline_reason(x, 0, "spatial", None, 600)
    assert "not two-dimensional" in _decline_reason(np.zeros((3, 42)), 0, "spatial", None, 4)
    assert "float64 is served" in _decline_reason(x.astype(np.float32), 0, "spatial", None, 4)


def test_patch_cycle_and_registration(ref_pysteps):
    from pysteps.timeseries import correlation as ref

    from pysteps_amd import register
    from pysteps_amd.timeseries import correlation

    stock = ref.temporal_autocorrelation
    multivariate = ref.temporal_autocorrelation_multivariate
    try:
        register.register()
        plain = register.register()  # with the FFT method in place already: what every later call returns
        assert ref.temporal_autocorrelation is stock and "correlation:temporal_autocorrelation" not in plain
        assert register.patch_correlation() == ["correlation:temporal_autocorrelation"]
        assert ref.temporal_autocorrelation is correlation.temporal_autocorrelation and ref._reference_temporal_autocorrelation is stock
        assert ref.temporal_autocorrelation_multivariate is multivariate
        assert register.patch_correlation() == []  # already in place
        register.unpatch_correlation()
        assert ref.temporal_autocorrelation is stock and not hasattr(ref, "_reference_temporal_autocorrelation")
        assert register.register(correlation=True) == plain + ["correlation:temporal_autocorrelation"]
        assert ref.temporal_autocorrelation is correlation.temporal_autocorrelation and ref._reference_temporal_autocorrelation is stock
        register.unpatch_correlation()
        register.unpatch_correlation()  # harmless when nothing is patched
        assert ref.temporal_autocorrelation is stock
    finally:
        register.unpatch_correlation()
        register.unregister_fft()


def test_a_declined_call_returns_the_stock_answer_with_the_warning(ref_pysteps, monkeypatch):
    from pysteps.timeseries import correlation as ref

    from pysteps_amd import _lib, register
    from pysteps_amd.timeseries import correlation

    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("a declined call must not touch the device"))
    x = (restated.cascade((5, 7), 1, 3, "float64")[0] * 8).astype(np.int64)
    want = ref.temporal_autocorrelation(x)
    try:
        register.patch_correlation()
        with pytest.warns(RuntimeWarning, match="dtype int64 .* running the reference's function"):
            got = ref.temporal_autocorrelation(x)
        assert got == want and len(got) == 2
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            assert correlation.temporal_autocorrelation(x, d=1) == ref._reference_temporal_autocorrelation(x, d=1)
    finally:
        register.unpatch_correlation()
