"""Radially averaged power spectra on the device (``pysteps_amd.utils.spectral``, csrc/rapsd.hip).

The binning is held to exact arithmetic (tests/helpers/rapsd.py: ``math.fsum`` per bin) with the counts equal as
integers and every bin mean within 5 x ``deviation_mean``, the distance the goldens' maker measured between the
reference's ``np.mean`` and the exact mean of the same terms (4.5e-16; the bar is 2.2e-15).  The same bar holds against
the reference's goldens where the transform is NumPy's on both sides.  Through the device transform the spectra are
held to the count-weighted sum ``sum_r N_r |got_r - want_r| <= 2.1e-12 sum_r N_r want_r``, which follows from the bar
tests/test_fft_gpu.py holds the transform to (rel-L2 <= 1e-12 against NumPy: ``|| |X|^2 - |Y|^2 ||_1 <= ||X - Y||_2
(||X||_2 + ||Y||_2)``); the per-bin figure there is printed, it would measure the chirp-z transform against pocketfft.
"""

import functools
import json
import os
import warnings

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import rapsd as restated

pytestmark = pytest.mark.gpu

PATH = os.path.join(GOLDEN, "rapsd_reference.npz")
SHAPES = {name: shape for name, (shape, _) in restated.CASES.items()}
SHAPES.update({"x%dx%d" % s: s for s in restated.EXTRA_SHAPES})
DTYPES = ["float32", "float64"]


@pytest.fixture(scope="module")
def golden():
    return np.load(PATH)


def bar_of(golden):
    return 5.0 * float(golden["deviation_mean"])


@functools.lru_cache(maxsize=None)
def field_of(name):
    """The float32 field of a case: the golden's for the golden shapes (test_rapsd_cpu.py holds the file to the same
    generator), a generated one for the others."""
    if name in restated.CASES:
        (m, n), seed = restated.CASES[name]
    else:
        (m, n), seed = SHAPES[name], 40 + list(SHAPES).index(name)
    field = restated.rain_field(m, n, seed)
    field.setflags(write=False)
    return field


@functools.lru_cache(maxsize=None)
def power_of(name, dtype):
    """A shifted power plane of the case and what exact arithmetic makes of it: (plane, means, counts)."""
    power = restated.shifted_power(field_of(name).astype(np.float64)).astype(dtype)
    power.setflags(write=False)
    return (power,) + restated.exact_full(power)


def upload(x):
    from pysteps_amd.device import DeviceArray

    return DeviceArray.from_host(np.ascontiguousarray(x))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_binning_is_exact(golden, name, dtype):
    from pysteps_amd.utils import fft, spectral

    bar = bar_of(golden)
    m, n = SHAPES[name]
    power, want, want_counts = power_of(name, dtype)
    np.testing.assert_array_equal(spectral.rapsd_counts((m, n)), want_counts)
    np.testing.assert_array_equal(spectral.rapsd_counts((m, n), half=True), want_counts)
    means, counts = spectral._full(upload(power[np.newaxis]))
    np.testing.assert_array_equal(counts.astype(np.int64), want_counts)
    assert means.dtype == np.float64 and means.shape == (1, want.size)
    for resident in (False, True):
        got = spectral.rapsd(upload(power) if resident else power)
        assert got.dtype == np.float64 and got.tobytes() == means[0].tobytes()
        worst = restated.relative(got, want)
        print("%s %s full plane, %s: %.3g of %.3g" % (name, dtype, "device" if resident else "numpy", worst, bar))
        assert worst <= bar

    field = field_of(name).astype(dtype)
    half_spectrum = fft.rfft2(upload(field.astype(np.float64)))  # resident in, resident out: complex128 as the kernel reads it
    assert half_spectrum.shape == (m, n // 2 + 1) and half_spectrum.dtype == np.complex128
    want, want_counts = restated.exact_half(np.array(half_spectrum.to_host()), m, n)
    np.testing.assert_array_equal(want_counts, power_of(name, dtype)[2])
    for resident in (False, True):
        got = spectral.rapsd(upload(field) if resident else field, fft_method="hip")
        worst = restated.relative(got, want)
        print("%s %s half spectrum, %s: %.3g of %.3g" % (name, dtype, "device" if resident else "numpy", worst, bar))
        assert got.dtype == np.float64 and worst <= bar
    assert spectral.rapsd(field, fft_method=fft.get_hip((m, n))).tobytes() == got.tobytes()


@pytest.mark.parametrize("name", list(restated.CASES))
def test_reference_goldens_through_numpy_fft(golden, name):
    from pysteps_amd.utils import spectral

    bar = bar_of(golden)
    field = golden[name + "__field"].astype(np.float64)
    d = float(golden["freq_d"])
    got, freq = spectral.rapsd(field, fft_method=np.fft, return_freq=True, d=d)
    assert freq.tobytes() == golden[name + "__freq"].tobytes() and freq.dtype == golden[name + "__freq"].dtype
    from_power = spectral.rapsd(restated.shifted_power(field))
    normalized = spectral.rapsd(field, fft_method=np.fft, normalize=True)
    figures = (restated.relative(got, golden[name + "__spectrum"]), restated.relative(from_power, golden[name + "__from_power"]),
               restated.relative(normalized, golden[name + "__normalized"]))
    print("%s: np.fft %.3g, from the power plane %.3g (bar %.3g), normalized %.3g (bar %.3g)"
          % (name, figures[0], figures[1], bar, figures[2], 2.0 * bar))
    assert figures[0] <= bar and figures[1] <= bar
    assert figures[2] <= 2.0 * bar  # a quotient of two such numbers
    assert got.shape == golden[name + "__spectrum"].shape and got.dtype == np.float64
    resident = spectral.rapsd(upload(field), fft_method=np.fft)
    assert resident.tobytes() == got.tobytes()


@pytest.mark.parametrize("name", list(restated.CASES))
def test_reference_goldens_through_the_device_transform(golden, name):
    from pysteps_amd.utils import spectral

    field = golden[name + "__field"].astype(np.float64)
    want, counts = golden[name + "__spectrum"], golden[name + "__counts"].astype(np.float64)
    got = spectral.rapsd(field, fft_method="hip")
    print("%s: per bin %.3g (not asserted: the two transforms), weighted %.3g of 2.1e-12"
          % (name, restated.relative(got, want), float(np.sum(counts * np.abs(got - want)) / np.sum(counts * want))))
    assert np.sum(counts * np.abs(got - want)) <= 2.1e-12 * np.sum(counts * want)
    normalized = spectral.rapsd(field, fft_method="hip", normalize=True)
    assert abs(float(np.sum(normalized)) - 1.0) <= 1e-14 and normalized.tobytes() == (got / np.sum(got)).tobytes()


def test_known_answers():
    from pysteps_amd.utils import spectral

    for m, n in [(32, 32), (64, 128)]:
        constant = restated.constant_field(m, n)
        for method in (np.fft, "hip"):
            got = spectral.rapsd(constant, fft_method=method)
            assert got[0] == 9.0 * m * n and not got[1:].any(), (m, n, method)
    plane = np.zeros((33, 40))
    plane[33 // 2, 40 // 2] = 7.0
    got = spectral.rapsd(plane)
    assert got[0] == 7.0 and not got[1:].any()
    for (m, n, a, b) in [(48, 64, 5, 3), (129, 140, 17, 30), (96, 50, 0, 11)]:
        peak = int(restated.bin_rule(a * a + b * b))
        cosine = restated.cosine_field(m, n, a, b)
        for method in (np.fft, "hip"):
            got = spectral.rapsd(cosine, fft_method=method)
            others = np.delete(got, peak)
            print("cosine %dx%d (%d, %d) %s: bin %d, largest other bin %.3g of it" % (m, n, a, b, method if method == "hip" else "np.fft",
                                                                                    peak, float(others.max() / got[peak])))
            assert got[peak] > 0 and np.all(others < 1e-20 * got[peak])
            count = spectral.rapsd_counts((m, n))[peak]
            assert abs(got[peak] * count - m * n / 2.0) <= 1e-12 * m * n


def test_table_rows_are_single_calls_and_runs_repeat():
    from pysteps_amd.utils import spectral

    m, n = 129, 140
    fields = np.stack([restated.rain_field(m, n, 60 + k) for k in range(7)])  # float32; odd rows: planes at every alignment
    singles = {method: [spectral.rapsd(fields[k], fft_method=method) for k in range(7)] for method in ("hip", None)}
    for method in ("hip", None):
        for K in (1, 3, 7):
            table = spectral.rapsd_table(fields[:K], fft_method=method)
            assert table.shape == (K, restated.bins(m, n)) and table.dtype == np.float64
            for k in range(K):
                assert table[k].tobytes() == singles[method][k].tobytes(), (method, K, k)
        whole = spectral.rapsd_table(upload(fields), fft_method=method)
        again = spectral.rapsd_table(upload(fields), fft_method=method)
        assert whole.tobytes() == again.tobytes()
        parts = np.concatenate([spectral.rapsd_table(fields[:3], fft_method=method), spectral.rapsd_table(fields[3:], fft_method=method)])
        assert parts.tobytes() == whole.tobytes()
        wide = spectral.rapsd_table(upload(fields.astype(np.float64)), fft_method=method)
        assert wide.tobytes() == whole.tobytes()  # float32 members are their float64 values
    normalized, freq = spectral.rapsd_table(fields, normalize=True, return_freq=True, d=2.0)
    for k in range(7):
        assert normalized[k].tobytes() == spectral.rapsd(fields[k], fft_method="hip", normalize=True).tobytes()
    assert freq.tobytes() == np.fft.fftfreq(140, d=2.0)[:70].tobytes()
    small_batches = spectral._BATCH_BYTES
    try:
        spectral._BATCH_BYTES = 2 * m * (n // 2 + 1) * 16  # two half spectra at a time: 2 + 2 + 2 + 1
        assert spectral.rapsd_table(fields).tobytes() == spectral.rapsd_table(upload(fields)).tobytes()
        spectral._BATCH_BYTES = small_batches
        assert spectral.rapsd_table(fields).tobytes() == np.stack(singles["hip"]).tobytes()
    finally:
        spectral._BATCH_BYTES = small_batches


def test_accumulator_driven_by_hand():
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.utils import spectral

    m, n = 129, 140
    members = np.stack([restated.rain_field(m, n, 70 + k) for k in range(6)]).reshape(2, 3, m, n)
    observations = np.stack([members[0, 1], restated.rain_field(m, n, 79)]).astype(np.float64)
    for resident in (True, False):
        acc = spectral.RapsdAccumulator(observations, per_member=True)
        assert acc.mean_spectra is None and acc.member_spectra is None
        for t in range(2):
            acc(upload(members[t]) if resident else members[t])
        assert acc.received == [DeviceArray if resident else np.ndarray] * 2 and acc.n_leadtimes == 2
        for t in range(2):
            table = spectral.rapsd_table(members[t])
            assert acc.mean_spectra[t].tobytes() == np.mean(table, axis=0).tobytes()
            assert acc.member_spectra[t].tobytes() == table.tobytes()
        assert acc.obs_spectra.tobytes() == spectral.rapsd_table(observations).tobytes()
        assert acc.ratio().shape == (2, 70) and acc.ratio().tobytes() == (acc.mean_spectra / acc.obs_spectra).tobytes()
        assert acc.freq(2.0).tobytes() == np.fft.fftfreq(140, d=2.0)[:70].tobytes()
        with pytest.raises(ValueError, match="called for more lead times than the 2 observations"):
            acc(members[0])
    same = spectral.RapsdAccumulator(upload(observations[:1]), normalize=True)
    same(np.stack([observations[0]] * 2))  # two members: their mean (s + s) / 2 is s without a rounding
    np.testing.assert_array_equal(same.ratio(), np.ones((1, 70)))
    assert same.member_spectra is None and abs(float(same.mean_spectra.sum()) - 1.0) < 1e-14
    with pytest.raises(ValueError, match=r"members of shape \(k, 129, 140\) expected, got \(3, 140, 129\)"):
        same(np.zeros((3, 140, 129)))
    with pytest.raises(ValueError, match=r"members of shape \(k, 129, 140\) expected, got \(129, 140\)"):
        same(observations[0])
    free = spectral.RapsdAccumulator()
    with pytest.raises(ValueError, match="no field seen yet"):
        free.freq()
    free(members[0])
    assert free.obs_spectra is None and free.mean_spectra.shape == (1, 70)
    with pytest.raises(ValueError, match="no observations given"):
        free.ratio()
    holes = members[1].copy()
    holes[:, :5, :] = np.nan
    with pytest.raises(ValueError, match="input field should not contain nans"):
        spectral.RapsdAccumulator()(holes)
    filled = spectral.RapsdAccumulator(nan_value=-1.5)
    filled(upload(holes))
    assert filled.mean_spectra[0].tobytes() == np.mean(spectral.rapsd_table(np.where(np.isnan(holes), -1.5, holes)), axis=0).tobytes()


def test_accumulator_inside_a_real_steps_run(ref_pysteps):
    """The real pysteps.nowcasts.steps with the resident loop and return_output=False: the accumulator receives the
    members where they lie and no member is downloaded."""
    from pysteps import nowcasts

    from pysteps_amd import register
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.nowcasts import utils as loop
    from pysteps_amd.utils import spectral
    from test_callers_gpu import _steps_inputs, _steps_kwargs

    frames, V = _steps_inputs(128, 128)  # the smallest shape the resident loop's tests run
    kw = _steps_kwargs()
    n_leadtimes = 2
    observations = np.stack([frames[-1]] * n_leadtimes)
    steps = nowcasts.get_method("steps")
    try:
        register.register(patch_main_loop=True)
        acc = spectral.RapsdAccumulator(observations, per_member=True, nan_value=float(np.nanmin(frames)))
        out = steps(frames, V, n_leadtimes, extrap_method="semilagrangian_hip", callback=acc, return_output=False, **kw)
        assert out is None and "download" not in loop.last_run_stats and "callback" in loop.last_run_stats
        assert acc.n_leadtimes == n_leadtimes and acc.received == [DeviceArray] * n_leadtimes
        assert acc.mean_spectra.shape == (n_leadtimes, 64) and np.isfinite(acc.mean_spectra).all() and acc.mean_spectra.min() > 0
        assert all(table.shape == (kw["n_ens_members"], 64) for table in acc.member_spectra)
        ratio = acc.ratio()
        print("ensemble-mean over observed power, lead time 1: largest scales %s, smallest scales %s" % (ratio[0, 1:4], ratio[0, -3:]))
        assert ratio.shape == (n_leadtimes, 64) and np.isfinite(ratio).all() and ratio.min() > 0
    finally:
        register.unpatch_main_loop()
        register.unregister_fft()


def test_declined_inputs_run_the_reference(ref_pysteps):
    from pysteps.utils import spectral as ref

    from pysteps_amd.utils import spectral

    reference = getattr(ref, "_reference_rapsd", ref.rapsd)
    with_inf = restated.rain_field(64, 80, 5).astype(np.float64)
    with_inf[3, 4] = np.inf
    long_side = restated.rain_field(5000, 64, 6).astype(np.float64)
    integers = np.arange(48 * 48, dtype=np.int32).reshape(48, 48) % 7
    for field, why in ((with_inf, "an infinite value"), (long_side, r"the shape \(5000, 64\)"), (integers, "a field of dtype int32")):
        with pytest.warns(RuntimeWarning, match="pysteps_amd rapsd: %s - running the reference's function" % why):
            got, freq = spectral.rapsd(field, fft_method=np.fft, return_freq=True, d=3.0)
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            want, want_freq = reference(field, fft_method=np.fft, return_freq=True, d=3.0)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(freq, want_freq)
    # "hip" is no object the reference could call: it stands for np.fft, the reference's default method, there
    for field, why in ((with_inf, "an infinite value"), (long_side, r"the shape \(5000, 64\)"), (integers, "a field of dtype int32")):
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            want = reference(field, fft_method=np.fft)
            want_normalized = reference(field, fft_method=np.fft, normalize=True)
        with pytest.warns(RuntimeWarning, match="pysteps_amd rapsd: %s - running the reference's function" % why):
            np.testing.assert_array_equal(spectral.rapsd(field, fft_method="hip"), want)
        stack = np.stack([field, field[::-1].copy()])
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            want_table = np.stack([want, reference(stack[1], fft_method=np.fft)])
        with pytest.warns(RuntimeWarning, match="pysteps_amd rapsd: %s - running the reference's function" % why):
            table = spectral.rapsd_table(stack)  # its default method
        np.testing.assert_array_equal(table, want_table)
        with pytest.warns(RuntimeWarning, match="running the reference's function"):
            np.testing.assert_array_equal(spectral.rapsd_table(stack[:1], normalize=True)[0], want_normalized)
        with pytest.warns(RuntimeWarning, match="pysteps_amd rapsd: %s - running the reference's function" % why):
            acc = spectral.RapsdAccumulator(per_member=True)
            acc(stack)  # host members
        np.testing.assert_array_equal(acc.member_spectra[0], want_table)
        with np.errstate(all="ignore"):
            np.testing.assert_array_equal(acc.mean_spectra[0], np.mean(want_table, axis=0))
    with pytest.warns(RuntimeWarning, match="a field of dtype int32"):
        filled = spectral.RapsdAccumulator(nan_value=0.0)
        filled(integers[np.newaxis])
    with pytest.raises(NotImplementedError, match="an infinite value is not implemented on the device"):
        spectral.rapsd(upload(with_inf), fft_method="hip")
    with pytest.raises(NotImplementedError, match="the shape"):
        spectral.rapsd_table(upload(long_side[np.newaxis]))


def test_nan_raises_the_reference_s_text(golden):
    from pysteps_amd.utils import spectral

    text = json.loads(str(golden["messages"]))["nan"]
    field = restated.rain_field(33, 47, 7)
    field[5, 6] = np.nan
    for method in (None, np.fft, "hip"):
        for x in (field, field.astype(np.float64), upload(field)):
            with pytest.raises(ValueError) as err:
                spectral.rapsd(x, fft_method=method)
            assert str(err.value) == text
    with pytest.raises(ValueError) as err:
        spectral.rapsd_table(np.stack([field, field]))
    assert str(err.value) == text


def test_registered_rapsd_serves_the_noise_filter(golden, ref_pysteps):
    """After register(rapsd=True) the reference's parametric noise filter takes its spectrum on the device: it looks
    ``utils.spectral.rapsd`` up when it is called (noise/fftgenerators.py:150, fft_method=None on a shifted plane)."""
    import pysteps.utils.spectral as ref_mod
    from pysteps.noise import fftgenerators

    from pysteps_amd import register
    from pysteps_amd.utils import spectral

    field = restated.power_law_field(128, 128, 8)
    reference = ref_mod.rapsd
    calls = []

    def recording(*args, **kwargs):
        calls.append((args, kwargs, spectral.rapsd(*args, **kwargs)))
        return calls[-1][2]

    try:
        register.register(fft=False, rapsd=True)
        assert ref_mod.rapsd is spectral.rapsd
        ref_mod.rapsd = recording
        got = fftgenerators.initialize_param_2d_fft_filter(field)
    finally:
        ref_mod.rapsd = spectral.rapsd
        register.unpatch_rapsd()
    assert len(calls) == 1 and ref_mod.rapsd is reference
    args, kwargs, served = calls[0]
    assert kwargs.get("fft_method") is None and len(args) == 1 and args[0].shape == (128, 128)
    assert restated.relative(served, reference(*args, **kwargs)) <= bar_of(golden)
    assert np.isfinite(got["field"]).all()
