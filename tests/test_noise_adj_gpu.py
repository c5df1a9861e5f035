"""The noise standard-deviation adjustment on the device (pysteps_amd/noise/utils.py, csrc/noise_adj.hip) against the
reference's ``compute_noise_stddev_adjs`` and its NumPy restatement.

Every tolerance is 5 x what the reference's own float64 arithmetic deviates from a longdouble evaluation of the same
expressions (``deviation_coeffs``, ``deviation_moments`` of tests/golden/noise_adj_reference.npz, measured by
tools/make_golden_noise_adj.py): the device is allowed the reference's rounding noise with room for another, equally
sound summation order.  What is element-wise or a matter of order alone is held to identical bits.
"""

import os
import warnings

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import noise_adj as restated

pytestmark = pytest.mark.gpu

_CASES = {}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "noise_adj_reference.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def bars(golden):
    return 5.0 * float(golden["deviation_coeffs"]), 5.0 * float(golden["deviation_moments"])


def _case(ref_pysteps, golden, name):
    """(R, F, noise_filter) of a case, made once."""
    if name not in _CASES:
        R = golden[name + "__R"].astype(np.float64)
        _CASES[name] = (R,) + restated.filters(ref_pysteps, R, restated.CASES[name][1])
    return _CASES[name]


def _ref_fns():
    from pysteps.cascade.decomposition import decomposition_fft
    from pysteps.noise.fftgenerators import generate_noise_2d_fft_filter
    from pysteps.noise.utils import compute_noise_stddev_adjs

    return compute_noise_stddev_adjs, decomposition_fft, generate_noise_2d_fft_filter


def _device(R, thr1, thr2, F, noise_filter, num_iter, conditional, seed, **kw):
    """the device path, with a declined call (RuntimeWarning) an error"""
    from pysteps_amd.noise import compute_noise_stddev_adjs

    _, decomp, generator = _ref_fns()
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message="pysteps_amd compute_noise_stddev_adjs", category=RuntimeWarning)
        return compute_noise_stddev_adjs(R, thr1, thr2, F, decomp, noise_filter, generator, num_iter, conditional=conditional,
                                         num_workers=1, seed=seed, **kw)


def _levels(R, thr1, thr2, weights):
    """the cascade levels of the centred observed field on the host (float64 NumPy) and the mask"""
    mask = R >= thr1
    x = R.copy()
    x[~mask] = thr2
    x -= np.mean(x[mask])
    spectrum = np.fft.rfft2(x)
    return np.stack([np.fft.irfft2(spectrum * weights[k], s=x.shape) for k in range(weights.shape[0])]), mask, x


@pytest.mark.parametrize("conditional", [True, False])
@pytest.mark.parametrize("name", sorted(restated.CASES))
def test_coefficients_match_the_reference_and_the_goldens(ref_pysteps, golden, bars, name, conditional):
    ref_fn, decomp, generator = _ref_fns()
    R, F, noise_filter = _case(ref_pysteps, golden, name)
    combos = [("wet",) + c for c in restated.COMBOS if c[0] == conditional]
    combos += [(mask,) + c for mask in ("sparse", "all") for c in restated.MASK_COMBOS if c[0] == conditional]
    seen = []
    for mask_kind, _, num_iter, seed in combos:
        thr1, thr2 = restated.thresholds(R, mask_kind)
        before = R.copy()
        got = _device(R, thr1, thr2, F, noise_filter, num_iter, conditional, seed)
        assert np.array_equal(R, before), "R was modified"
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (restated.CASES[name][1],)
        live = np.asarray(ref_fn(R, thr1, thr2, F, decomp, noise_filter, generator, num_iter, conditional=conditional, seed=seed))
        stored = golden[restated.key(name, mask_kind, conditional, num_iter, seed) + "__ref"]
        seen.append((mask_kind, num_iter, seed, restated.rel_dev(got, live), restated.rel_dev(got, stored)))
    print("\n%s conditional=%s bar %.3g: (mask, num_iter, seed, vs live, vs golden) %s" % (name, conditional, bars[0], seen))
    for mask_kind, num_iter, seed, vs_live, vs_stored in seen:
        assert vs_live <= bars[0] and vs_stored <= bars[0], (name, conditional, mask_kind, num_iter, seed, vs_live, vs_stored, bars[0])


@pytest.mark.parametrize("name", sorted(restated.CASES))
def test_masked_moments_stage(ref_pysteps, golden, bars, name):
    """psh_masked_moments_dev alone against np.mean(x[mask]) / np.std(x[mask]), relative to the plane's std"""
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.noise import utils as hip_mod

    R, F, _ = _case(ref_pysteps, golden, name)
    seen = []
    for mask_kind in restated.MASKS:
        thr1, thr2 = restated.thresholds(R, mask_kind)
        levels, mask, _ = _levels(R, thr1, thr2, F["weights_2d"])
        d_levels = DeviceArray.from_host(levels)
        d_mask = DeviceArray.from_host(mask.astype(np.uint8))
        count = hip_mod.mask_count(d_mask)
        assert int(count.to_host()[0]) == int(np.count_nonzero(mask))
        if mask_kind == "sparse":
            assert int(np.count_nonzero(mask)) < 64
        got = hip_mod.masked_moments(d_levels, d_mask, count, planes_per_block=4).to_host()
        one = hip_mod.masked_moments(d_levels, d_mask, count, planes_per_block=1).to_host()
        assert np.array_equal(got, one), "planes per block changes the bits"
        single = hip_mod.masked_moments(d_levels.view(levels.shape[0] - 1), d_mask).to_host()
        assert np.array_equal(single[0], got[-1]), "a plane's moments depend on its neighbours"
        for k in range(levels.shape[0]):
            sd = np.std(levels[k])
            sel = levels[k][mask]
            seen.append((mask_kind, k, abs(got[k, 0] - np.mean(sel)) / sd, abs(got[k, 1] - np.std(sel)) / sd))
    print("\n%s bar %.3g: (mask, level, mean, std) %s" % (name, bars[1], seen))
    for mask_kind, k, dmean, dstd in seen:
        assert dmean <= bars[1] and dstd <= bars[1], (name, mask_kind, k, dmean, dstd, bars[1])


def test_masked_moments_of_an_empty_mask_are_nan():
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.noise import utils as hip_mod

    x = DeviceArray.from_host(np.arange(67.0 * 5).reshape(67, 5))
    mask = DeviceArray((67, 5), np.uint8).fill_bytes(0)
    assert np.all(np.isnan(hip_mod.masked_moments(x, mask).to_host()))


@pytest.mark.parametrize("name", sorted(restated.CASES))
def test_spectrum_level_moments_stage(ref_pysteps, golden, bars, name):
    """psh_spectrum_level_moments_dev against the spatial route on the device (levels by inverse transforms, moments
    over an all-ones mask) on the same field, and against NumPy on the host"""
    from pysteps_amd import _lib
    from pysteps_amd.cascade.decomposition import _device_weights
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.noise import utils as hip_mod
    from pysteps_amd.utils import fft as hip_fft

    R, F, _ = _case(ref_pysteps, golden, name)
    m, n = R.shape
    L = F["weights_2d"].shape[0]
    assert hip_mod._self_conjugate_columns_symmetric(F["weights_2d"], n)
    thr1, thr2 = restated.thresholds(R, "wet")
    host_levels, _, x = _levels(R, thr1, thr2, F["weights_2d"])
    d_x = DeviceArray.from_host(np.stack([x, np.roll(x, 3, axis=1) * 0.5 + 1.0]))
    weights = _device_weights(F["weights_2d"])
    spectra = DeviceArray((2, m, n // 2 + 1), np.complex128)
    for j in range(2):
        _lib.check(_lib.lib().psh_fft_rfft2_dev(d_x.view(j).ptr, m, n, spectra.view(j).ptr), "psh_fft_rfft2_dev")
    spectral = hip_mod.spectrum_level_moments(spectra, weights, (m, n)).to_host()
    alone = hip_mod.spectrum_level_moments(spectra.view(1), weights, (m, n)).to_host()
    assert np.array_equal(alone[0], spectral[1]), "a spectrum's moments depend on the batch"
    ones = DeviceArray((m, n), np.uint8).fill_bytes(1)
    seen = []
    for j in range(2):
        levels = DeviceArray((L, m, n), np.float64)
        _lib.check(_lib.lib().psh_cascade_decompose_levels_dev(d_x.view(j).ptr, weights.ptr, L, m, n, levels.ptr),
                   "psh_cascade_decompose_levels_dev")
        spatial = hip_mod.masked_moments(levels, ones).to_host()
        for k in range(L):
            sd = spatial[k, 1]
            seen.append((j, k, abs(spectral[j, k, 0] - spatial[k, 0]) / sd, abs(spectral[j, k, 1] - spatial[k, 1]) / sd))
    for k in range(L):  # and the host's levels of the first field
        sd = np.std(host_levels[k])
        seen.append(("host", k, abs(spectral[0, k, 0] - np.mean(host_levels[k])) / sd, abs(spectral[0, k, 1] - sd) / sd))
    print("\n%s bar %.3g: (field, level, mean, std) %s" % (name, bars[1], seen))
    for j, k, dmean, dstd in seen:
        assert dmean <= bars[1] and dstd <= bars[1], (name, j, k, dmean, dstd, bars[1])
    assert hip_fft.supported_shape((m, n))


@pytest.mark.parametrize("name", sorted(restated.CASES))
def test_prepare_stage_is_the_numpy_expression(ref_pysteps, golden, bars, name):
    """psh_noise_adj_prepare_dev against utils.py:113-118, operation by operation.  The bar is EXACT for the element-wise
    part: with the standard deviation the device divided by, every value has the bits of the NumPy expression.  The
    standard deviation itself is a reduction in another (equally sound) order than np.std's pairwise one, so it is held
    to 5 x deviation_moments instead (relative to the plane's std, which it is)."""
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.noise import utils as hip_mod

    R, F, noise_filter = _case(ref_pysteps, golden, name)
    thr1, thr2 = restated.thresholds(R, "wet")
    mask = R >= thr1
    sigma, mu = float(np.std(R[mask])), float(np.mean(R[mask]))
    rs = restated.seed_chain(3, 3)
    fields = np.stack([restated.filtered_noise(r, noise_filter["field"], R.shape, np.float64) for r in rs])
    fields[2] = fields[2] * 3.0 + 0.25  # not standardised: the division matters
    d_fields = DeviceArray.from_host(fields)
    d_mask = DeviceArray.from_host(mask.astype(np.uint8))
    stats = DeviceArray((3, 2), np.float64)
    hip_mod.prepare(d_fields, d_mask, sigma, mu, thr2, stats_out=stats)
    got, used = d_fields.to_host(), stats.to_host()
    for j in range(3):
        sd = np.std(fields[j])
        assert abs(used[j, 1] - sd) / sd <= bars[1], (j, used[j, 1], sd)
        N = fields[j] / used[j, 1] * sigma + mu
        N[~mask] = thr2
        N -= mu
        assert np.array_equal(got[j], N), (name, j, int(np.count_nonzero(got[j] != N)))
    alone = DeviceArray.from_host(fields[1:2])
    hip_mod.prepare(alone, d_mask, sigma, mu, thr2)
    assert np.array_equal(alone.to_host()[0], got[1]), "a field's result depends on the batch"


def test_observed_field_stage(ref_pysteps, golden):
    """utils.py:83-87 and :92 on a field with NaN and infinities"""
    from pysteps_amd import _lib
    from pysteps_amd.device import DeviceArray

    R = golden["o67x129__R"].astype(np.float64)
    R[3, 5:9], R[10, 2], R[11, 3] = np.nan, np.inf, -np.inf
    thr1, thr2 = -10.0, -15.0
    mask = R >= thr1
    want = R.copy()
    want[~np.isfinite(want)] = thr2
    want[~mask] = thr2
    d_R = DeviceArray.from_host(R)
    d_mask, d_clean = DeviceArray(R.shape, np.uint8), DeviceArray(R.shape, np.float64)
    _lib.check(_lib.lib().psh_noise_adj_observed_dev(d_R.ptr, R.size, thr1, thr2, d_mask.ptr, d_clean.ptr), "observed")
    assert np.array_equal(d_mask.to_host().astype(bool), mask) and np.array_equal(d_clean.to_host(), want)
    _lib.check(_lib.lib().psh_noise_adj_centre_dev(d_clean.ptr, R.size, 1.75), "centre")
    assert np.array_equal(d_clean.to_host(), want - 1.75)
    assert np.array_equal(d_R.to_host(), R, equal_nan=True)


@pytest.mark.parametrize("conditional", [True, False])
def test_exactness_without_tolerance(ref_pysteps, golden, conditional):
    """two calls, batches of 1 and 2 realisations, a resident input: identical bits; the device generators end where
    host generators that drew the same fields end; R is unchanged"""
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.noise import utils as hip_mod

    name = "e96x130"
    R, F, noise_filter = _case(ref_pysteps, golden, name)
    m, n = R.shape
    L = restated.CASES[name][1]
    thr1, thr2 = restated.thresholds(R, "wet")
    before = R.copy()
    states = []
    first = _device(R, thr1, thr2, F, noise_filter, 5, conditional, 42, _randstates_out=states)
    again = _device(R, thr1, thr2, F, noise_filter, 5, conditional, 42)
    assert np.array_equal(first, again) and np.all(np.isfinite(first))
    per = hip_mod._per_realisation_bytes(m, n, L, not conditional)
    for k in (1, 2):
        batched = _device(R, thr1, thr2, F, noise_filter, 5, conditional, 42, _batch_bytes=k * per)
        assert np.array_equal(first, batched), "batches of %d" % k
    resident = _device(DeviceArray.from_host(R), thr1, thr2, F, noise_filter, 5, conditional, 42)
    assert np.array_equal(first, resident)
    assert np.array_equal(R, before)
    host = restated.seed_chain(42, 5)
    assert len(states) == 5
    for ours, theirs in zip(states, host):
        theirs.randn(m, n)
        a, b = ours.get_state(legacy=True), theirs.get_state(legacy=True)
        assert np.array_equal(a[1], b[1]) and a[2:4] == b[2:4] and (a[3] == 0 or a[4] == b[4])


def test_fallback_to_spatial_levels_for_weights_that_are_not_symmetric(ref_pysteps, golden, bars):
    """band-pass weights that fail the self-conjugate-column check keep the spatial route (levels + moments over an
    all-ones mask) for conditional=False; the reference agrees"""
    from pysteps_amd.noise import utils as hip_mod

    ref_fn, decomp, generator = _ref_fns()
    R, F, noise_filter = _case(ref_pysteps, golden, "p64x64")
    F2 = dict(F)
    F2["weights_2d"] = F["weights_2d"].copy()
    F2["weights_2d"][1, 5, 0] *= 1.5  # (5, 0) and (59, 0) now differ on the self-conjugate column
    assert not hip_mod._self_conjugate_columns_symmetric(F2["weights_2d"], 64)
    thr1, thr2 = restated.thresholds(R, "wet")
    got = _device(R, thr1, thr2, F2, noise_filter, 3, False, 0)
    want = np.asarray(ref_fn(R, thr1, thr2, F2, decomp, noise_filter, generator, 3, conditional=False, seed=0))
    assert restated.rel_dev(got, want) <= bars[0], (got, want)


def test_seed_none_runs_and_leaves_the_global_generator_alone(ref_pysteps, golden):
    R, F, noise_filter = _case(ref_pysteps, golden, "p64x64")
    thr1, thr2 = restated.thresholds(R, "wet")
    np.random.seed(9)
    before = np.random.get_state()
    got = _device(R, thr1, thr2, F, noise_filter, 2, True, None)
    after = np.random.get_state()
    assert got.shape == (restated.CASES["p64x64"][1],) and np.all(np.isfinite(got))
    assert np.array_equal(before[1], after[1]) and before[2:] == after[2:]


def test_steps_end_to_end_with_the_patched_adjustment(ref_pysteps, bars):
    """the real nowcasts.steps with noise_stddev_adj="auto" after register(patch_main_loop=True, noise_stddev_adj=True):
    the patched function is the one called, on the device path; its coefficients meet the coefficient bar against the
    stock function's on the very arguments steps hands over, and the forecast the end-to-end bar of
    tests/test_steps_resident_gpu.py.  (The coefficients of the stock RUN are not the yardstick: steps builds the noise
    filter from the advected input frames (steps.py:697 before :746), and the stock run advects them with the stock
    extrapolator - its filter differs from this run's at single-precision rounding, 2e-8 in the coefficients.)"""
    import pysteps.noise.utils as ref_mod
    from pysteps import nowcasts

    from pysteps_amd import register
    from pysteps_amd.noise import utils as hip_mod
    from test_callers_gpu import _ensemble_close
    from tools import synth

    frames = synth.steps_frames(64, 64, 3).astype(np.float64)
    V = synth.true_velocity(64, 64).astype(np.float64)
    kw = dict(n_ens_members=2, n_cascade_levels=3, precip_thr=-10.0, kmperpixel=1.0, timestep=5.0, seed=42, vel_pert_method="bps",
              mask_method="incremental", probmatching_method="cdf", num_workers=1, noise_stddev_adj="auto")
    steps = nowcasts.get_method("steps")
    stock_fn = ref_mod.compute_noise_stddev_adjs
    assert stock_fn is not hip_mod.compute_noise_stddev_adjs
    coeffs = {}

    def recording(label, fn):
        def call(*args, **kwargs):
            with warnings.catch_warnings():  # a declined call is an error here
                warnings.filterwarnings("error", message="pysteps_amd compute_noise_stddev_adjs", category=RuntimeWarning)
                coeffs[label] = np.asarray(fn(*args, **kwargs))
            if fn is not stock_fn:
                coeffs["stock_same_arguments"] = np.asarray(stock_fn(*args, **kwargs))
            return coeffs[label]

        return call

    try:
        ref_mod.compute_noise_stddev_adjs = recording("stock", stock_fn)
        want = steps(frames, V, 2, extrap_method="semilagrangian", **kw)
    finally:
        ref_mod.compute_noise_stddev_adjs = stock_fn
    try:
        added = register.register(patch_main_loop=True, noise_stddev_adj=True)
        assert "noise.utils:compute_noise_stddev_adjs" in added
        assert ref_mod.compute_noise_stddev_adjs is hip_mod.compute_noise_stddev_adjs
        ref_mod.compute_noise_stddev_adjs = recording("device", hip_mod.compute_noise_stddev_adjs)
        got = steps(frames, V, 2, extrap_method="semilagrangian_hip", **kw)
    finally:
        ref_mod.compute_noise_stddev_adjs = hip_mod.compute_noise_stddev_adjs
        register.unpatch_noise_stddev_adj()
        register.unpatch_main_loop()
    assert ref_mod.compute_noise_stddev_adjs is stock_fn
    assert set(coeffs) == {"stock", "device", "stock_same_arguments"} and coeffs["device"].shape == (3,)
    assert restated.rel_dev(coeffs["device"], coeffs["stock_same_arguments"]) <= bars[0], coeffs
    assert restated.rel_dev(coeffs["device"], coeffs["stock"]) <= 1e-6, coeffs  # the same adjustment, up to the extrapolators
    rel = _ensemble_close(got, want)
    assert rel < 1e-4, rel
