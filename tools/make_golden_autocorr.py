"""Golden vectors for the temporal autocorrelation and the AR estimate (``pysteps_amd.timeseries``), written by the
UNMODIFIED reference.

    python tools/make_golden_autocorr.py        (-> tests/golden/autocorr_reference.npz)

Runs pysteps/timeseries/correlation.py ``temporal_autocorrelation`` and pysteps/timeseries/autoregression.py
``adjust_lag2_corrcoef1/2``, ``estimate_ar_params_yw`` and ``test_ar_stationarity`` of the reference package that
``oracle.build_ref`` prepares under oracle/_ref, on the cases of tests/helpers/autocorr.py.  The file holds

* the small inputs: the level-0 float64 series of the 5 x 7 and 61 x 67 cases as generated (``series_<shape>``; the
  generator is integer arithmetic and is held to them) and the rfft2 half spectra the spectral cases are built from
  (``spec_<shape>``; transforms are not reproducible to the bit across machines, so they are stored);
* per spatial and spectral case the reference's coefficients ``<case>__ref`` (levels, lags) and the exact restatement
  ``<case>__exact`` (integer / rational sums, the finish in ``numpy.longdouble``), for the spectral cases also the
  exact spatial coefficients of the same fields ``<case>__spatial``;
* per moving-window case the reference's planes ``<case>__ref``;
* the AR estimate's outputs, the reference's ``RuntimeError`` text and the messages of the four argument checks;
* per spatial case with one or two lags the AR parameters of the chain of nowcasts/steps.py:834-866, ``<case>__phi``.

Three numbers say how far the reference's float64 arithmetic is from the numbers it stands for: ``deviation_spatial``
and ``deviation_spectral`` - the largest absolute difference between ``__ref`` and ``__exact`` over the spatial and
the spectral cases (the coefficients lie in [-1, 1]: the bars are absolute) - and ``deviation_phi`` -
``deviation_spatial`` times the largest row sum of |d phi / d gamma| of the chain over the ``__phi`` cases, i.e. what
that deviation of every coefficient can move an AR parameter.  The tests allow 5 x these.  The float64 restatement of
the helpers is checked against the reference bit for bit on the way.  Needs the reference; never runs on the GPU
machine.  Data only.
"""
import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUT = os.path.join(ROOT, "tests", "golden", "autocorr_reference.npz")


def quiet(fn, *args, **kwargs):
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*args, **kwargs)


def message_of(fn, *args, **kwargs):
    try:
        fn(*args, **kwargs)
    except Exception as exc:  # noqa: BLE001
        return [type(exc).__name__, str(exc)]
    raise AssertionError("no exception")


def main():
    import scipy

    from helpers import autocorr as restated
    from oracle import build_ref

    build_ref.build()
    build_ref.activate()
    from pysteps.timeseries import autoregression, correlation

    ref_fn = correlation.temporal_autocorrelation
    out = {"versions": np.array(json.dumps({"numpy": np.__version__, "scipy": scipy.__version__}))}

    def steps_chain(gamma):  # nowcasts/steps.py:847-866 for one level
        gamma = np.array(gamma, dtype=np.float64)
        if gamma.size == 2:
            gamma[1] = autoregression.adjust_lag2_corrcoef2(gamma[0], gamma[1])
        return gamma, autoregression.estimate_ar_params_yw(gamma)

    # ---- inputs -----------------------------------------------------------------------------------------------
    for shape in restated.STORED_SHAPES:
        out["series_%dx%d" % shape] = restated.cascade(shape, 1, 4, "float64")[0]
    spectra = {}
    for shape in restated.SPECTRAL_SHAPES:
        fields = restated.cascade(shape, 1, 4, "float64")[0]
        spectra[shape] = np.fft.rfft2(fields)
        out["spec_%dx%d" % shape] = spectra[shape]

    # ---- global spatial coefficients --------------------------------------------------------------------------
    dev_spatial = dev_phi_slope = 0.0
    names = []
    for name, shape, L, T, d, dtype, kind, variant in restated.spatial_cases():
        x = restated.cascade(shape, L, T, dtype, variant)
        mask = restated.mask_of(kind, shape)
        K = T - d - 1
        ref = np.array([quiet(ref_fn, x[l], d=d, mask=mask) for l in range(L)], dtype=np.float64).reshape(L, K)
        same = np.array([restated.reference_float64(x[l], d=d, mask=mask) for l in range(L)], dtype=np.float64).reshape(L, K)
        assert np.array_equal(ref, same, equal_nan=True), name
        exact = np.array([restated.exact_gamma(x[l], d, mask, dtype) for l in range(L)], dtype=np.float64).reshape(L, K)
        dev_spatial = max(dev_spatial, restated.max_abs_dev(ref, exact))
        out[name + "__ref"], out[name + "__exact"] = ref, exact
        names.append(name)
        enough = mask is None or int(mask.sum()) >= 8  # two pixels correlate to +-1: the Yule-Walker matrix is singular
        if d == 0 and K in (1, 2) and variant == "plain" and kind in ("none", "all", "sparse") and enough:
            out[name + "__phi"] = np.array([steps_chain(ref[l])[1] for l in range(L)])
            for l in range(L):
                dev_phi_slope = max(dev_phi_slope, restated.yw_bound(ref[l], lambda g: steps_chain(g)[1]))
    out["spatial_cases"] = np.array(names)

    # ---- spectral coefficients --------------------------------------------------------------------------------
    dev_spectral = 0.0
    names = []
    for name, shape, L, T, d, full in restated.spectral_cases():
        x = restated.spectral_cascade(spectra[shape], L, T, full, shape[1])
        fields = restated.cascade(shape, 1, 4, "float64")[0]
        K = T - d - 1
        ref = np.array([quiet(ref_fn, x[l], d=d, domain="spectral", x_shape=shape, use_full_fft=full) for l in range(L)],
                       dtype=np.float64).reshape(L, K)
        same = np.array([restated.reference_float64(x[l], d=d, domain="spectral", x_shape=shape, use_full_fft=full) for l in range(L)],
                        dtype=np.float64).reshape(L, K)
        assert np.array_equal(ref, same, equal_nan=True), name
        exact = np.array([restated.exact_gamma_spectral(x[l], d, shape, full) for l in range(L)], dtype=np.float64).reshape(L, K)
        spatial = np.array([restated.exact_gamma(np.stack([fields[(t + l) % 4] for t in range(T)]), d, None, "float64") for l in range(L)],
                           dtype=np.float64).reshape(L, K)
        dev_spectral = max(dev_spectral, restated.max_abs_dev(ref, exact))
        out[name + "__ref"], out[name + "__exact"], out[name + "__spatial"] = ref, exact, spatial
        names.append(name)
    out["spectral_cases"] = np.array(names)

    # ---- moving window ----------------------------------------------------------------------------------------
    names = []
    series = out["series_%dx%d" % restated.WINDOW_SHAPE]
    for name, T, d, sigma, masked in restated.window_cases():
        x = series[:T]
        mask = restated.window_mask(restated.WINDOW_SHAPE) if masked else None
        ref = np.array(quiet(ref_fn, x, d=d, mask=mask, window_radius=sigma))
        same = np.array(quiet(restated.reference_float64, x, d=d, mask=mask, window_radius=sigma))
        assert np.array_equal(ref, same, equal_nan=True), name
        uniform = np.array(quiet(ref_fn, x, d=d, mask=mask, window="uniform", window_radius=sigma))
        assert np.array_equal(ref, uniform, equal_nan=True), name  # the reference never passes window= on
        if masked:
            assert np.isnan(ref[:, :6, :8]).all(), name  # the two-pixel island
        # n is the window's weight over the mask times sigma**2: at most 2.25 for sigma = 1.5, which fails n >= 3 everywhere
        assert np.isnan(ref).all() == (sigma == 1.5), name
        out[name + "__ref"] = ref
        names.append(name)
    out["window_cases"] = np.array(names)

    # ---- the AR estimate --------------------------------------------------------------------------------------
    gammas = np.array(restated.AR_GAMMAS, dtype=np.float64)
    out["ar_adjust1"] = np.array([autoregression.adjust_lag2_corrcoef1(g[0], g[1]) for g in gammas])
    out["ar_adjust2"] = np.array([autoregression.adjust_lag2_corrcoef2(g[0], g[1]) for g in gammas])
    for p in (1, 2, 3):
        for d in (0, 1):
            rows, raised = [], []
            for g in gammas:
                try:
                    rows.append(autoregression.estimate_ar_params_yw(g[:p], d=d))
                    raised.append(False)
                except RuntimeError:
                    rows.append(np.full(p + d + 1, np.nan))
                    raised.append(True)
            out["ar_yw_p%d_d%d" % (p, d)], out["ar_yw_raised_p%d_d%d" % (p, d)] = np.array(rows), np.array(raised)
        unchecked = np.array([autoregression.estimate_ar_params_yw(g[:p], check_stationarity=False) for g in gammas])
        out["ar_yw_unchecked_p%d" % p] = unchecked
        out["ar_stationary_p%d" % p] = np.array([autoregression.test_ar_stationarity(row[:p]) for row in unchecked])
    messages = {
        "nonstationary": message_of(autoregression.estimate_ar_params_yw, np.array(restated.AR_NONSTATIONARY)),
        "yw_d": message_of(autoregression.estimate_ar_params_yw, gammas[0], d=2),
        "dimension": message_of(ref_fn, np.zeros(5)),
        "spectral": message_of(ref_fn, np.zeros((3, 2, 4, 4), dtype=complex), domain="spectral"),
        "mask": message_of(ref_fn, np.zeros((3, 4, 5)), mask=np.ones((4, 4), dtype=bool)),
        "nonfinite": message_of(ref_fn, np.full((3, 4, 5), np.nan)),
    }
    out["messages"] = np.array(json.dumps(messages))

    out["deviation_spatial"], out["deviation_spectral"] = np.float64(dev_spatial), np.float64(dev_spectral)
    out["deviation_phi"] = np.float64(dev_spatial * dev_phi_slope)
    np.savez_compressed(OUT, **out)
    print("%s: %d spatial, %d spectral, %d window cases, %.1f KiB; the reference deviates from the exact coefficients by "
          "%.3g (spatial) and %.3g (spectral); |d phi / d gamma| <= %.3g, deviation_phi %.3g"
          % (OUT, len(out["spatial_cases"]), len(out["spectral_cases"]), len(out["window_cases"]), os.path.getsize(OUT) / 1024.0,
             dev_spatial, dev_spectral, dev_phi_slope, dev_spatial * dev_phi_slope))


if __name__ == "__main__":
    main()
