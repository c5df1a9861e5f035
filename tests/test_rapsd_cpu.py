"""The host side of the radially averaged power spectrum (``pysteps_amd.utils.spectral``): the restatement the device
tests compare with (tests/helpers/rapsd.py) against the goldens of the unmodified reference, the two facts the kernels
rest on - the bin is an integer function of kx**2 + ky**2, the weighted half spectrum has the sums and counts of the
full plane - and the parts of the public interface that need no GPU."""

import inspect
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import rapsd as restated

PATH = os.path.join(GOLDEN, "rapsd_reference.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(PATH)


def case_names():
    return list(restated.CASES)


def field_of(golden, name):
    return golden[name + "__field"].astype(np.float64)


def test_golden_fields_are_the_helper_fields(golden):
    assert list(golden["cases"]) == case_names()
    for name, ((m, n), seed) in restated.CASES.items():
        assert golden[name + "__field"].dtype == np.float32
        np.testing.assert_array_equal(golden[name + "__field"], restated.rain_field(m, n, seed))
        assert golden[name + "__spectrum"].shape == (restated.bins(m, n),)


@pytest.mark.parametrize("name", case_names())
def test_restatement_counts_and_means_against_the_goldens(golden, name):
    power = restated.shifted_power(field_of(golden, name))
    means, counts = restated.exact_full(power)
    np.testing.assert_array_equal(counts, golden[name + "__counts"])
    assert counts.min() > 0
    assert golden[name + "__from_power"].tobytes() == golden[name + "__spectrum"].tobytes()
    worst = restated.relative(golden[name + "__spectrum"], means)
    print("%s: reference against the exact means %.3g (bar %.3g)" % (name, worst, float(golden["deviation_mean"])))
    assert worst <= float(golden["deviation_mean"])  # the maker measured it on these cases


@pytest.mark.parametrize("name", case_names())
def test_half_spectrum_has_the_sums_and_counts_of_the_full_plane(golden, name):
    field = field_of(golden, name)
    m, n = field.shape
    full, full_counts = restated.exact_full(restated.shifted_power(field))
    half, half_counts = restated.exact_half(np.fft.rfft2(field), m, n)
    np.testing.assert_array_equal(half_counts, full_counts)
    worst = restated.relative(half, full)
    print("%s: half against full %.3g" % (name, worst))
    assert worst <= 1e-13  # the rounding of two transforms of NumPy's, nothing of this project's


def test_integer_bin_rule_is_numpy_round_of_sqrt():
    """Every N a side up to 8192 can produce is at most 2 * 4096**2; all integers up to there are checked."""
    top = 2 * 4096 * 4096
    closest = 1.0
    for start in range(0, top + 1, 1 << 22):
        N = np.arange(start, min(start + (1 << 22), top + 1), dtype=np.int64)
        root = np.sqrt(N.astype(np.float64))
        np.testing.assert_array_equal(restated.bin_rule(N), np.round(root).astype(np.int64))
        closest = min(closest, float(np.min(np.abs(root - np.floor(root) - 0.5))))
    # (r + 1/2)**2 = r**2 + r + 1/4 is no integer: sqrt(N) stays 1 / (8 r) away from a tie, 2.1e-5 at the largest radius,
    # against 6e-13 of rounding in the square root - np.round never sees a tie
    assert closest > 2e-5
    r = restated.bin_rule(np.arange(0, 100000))
    N = np.arange(0, 100000)
    assert np.all((r * r - r < N) | (N == 0)) and np.all(N <= r * r + r)


def test_radius_grids_follow_the_integer_rule():
    for m, n in [(8, 8), (9, 9), (8, 9), (9, 8), (2, 64), (64, 3), (129, 140)]:
        yc, xc = restated.centred(m)[:, None], restated.centred(n)[None, :]
        np.testing.assert_array_equal(restated.r_grid_full(m, n), restated.bin_rule(xc * xc + yc * yc))


def test_known_answers_of_the_restatement():
    m, n, a, b = 48, 64, 5, 3
    means, counts = restated.exact_full(restated.shifted_power(restated.cosine_field(m, n, a, b)))
    peak = int(restated.bin_rule(a * a + b * b))
    others = np.delete(means, peak)
    assert means[peak] > 0 and np.all(others < 1e-20 * means[peak])
    assert abs(means[peak] * counts[peak] - m * n / 2.0) < 1e-9 * m * n  # two coefficients of (m n / 2)**2 / (m n)
    means, _ = restated.exact_full(restated.shifted_power(restated.constant_field(32, 32)))
    assert means[0] == 9.0 * 32 * 32 and not means[1:].any()


def test_signature_is_the_reference_s():
    from pysteps_amd.utils import spectral

    want = "(field, fft_method=None, return_freq=False, d=1.0, normalize=False, **fft_kwargs)"
    assert str(inspect.signature(spectral.rapsd)) == want
    from oracle import build_ref

    if build_ref.available() or build_ref.build() is not None:
        build_ref.activate()
        from pysteps.utils import spectral as ref

        assert inspect.signature(spectral.rapsd) == inspect.signature(getattr(ref, "_reference_rapsd", ref.rapsd))


def test_error_texts_are_the_goldens(golden):
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.utils import spectral

    messages = json.loads(str(golden["messages"]))
    assert set(messages) == {"ndim", "nan"}
    with pytest.raises(ValueError) as err:
        spectral.rapsd(np.zeros((2, 3, 4)))
    assert str(err.value) == messages["ndim"]
    with pytest.raises(ValueError) as err:
        spectral.rapsd(DeviceArray((2, 3, 4), np.float64, ptr=16))  # a handle is enough: the check comes first
    assert str(err.value) == messages["ndim"]
    with pytest.raises(ValueError, match="fields of shape"):
        spectral.rapsd_table(np.zeros((4, 4)))
    with pytest.raises(ValueError, match=r"observations of shape \(n_leadtimes, m, n\) expected, got \(4, 4\)"):
        spectral.RapsdAccumulator(np.zeros((4, 4)))
    # the NaN text is raised after the device has looked at the field: tests/test_rapsd_gpu.py
    assert messages["nan"] == "input field should not contain nans"


def test_exports_and_marker():
    import pysteps_amd.utils as utils
    from pysteps_amd.utils import fft, spectral

    assert utils.rapsd is spectral.rapsd and utils.rapsd_table is spectral.rapsd_table
    assert utils.RapsdAccumulator is spectral.RapsdAccumulator and spectral.RapsdAccumulator.accepts_device is True
    method = fft.get_hip((64, 64))
    assert method.pysteps_amd_hip is True and spectral._is_hip(method) and spectral._is_hip("hip")
    assert not spectral._is_hip(np.fft) and not spectral._is_hip(None) and not spectral._is_hip("numpy")
    assert [spectral._bins(*s) for s in [(8, 8), (9, 9), (8, 9), (2, 64), (640, 710)]] == [4, 5, 5, 32, 355]
    np.testing.assert_array_equal(spectral._freq(8, 9, 2.5), np.fft.fftfreq(9, d=2.5)[:5])


def test_register_swaps_and_restores_the_attribute(ref_pysteps):
    import pysteps.utils.spectral as ref_mod
    from pysteps import utils as ref_utils

    from pysteps_amd import register
    from pysteps_amd._reference import lookup
    from pysteps_amd.utils import spectral

    original = ref_mod.rapsd
    assert original is not spectral.rapsd
    try:
        added = register.register(fft=False)
        assert ref_mod.rapsd is original and "utils.spectral:rapsd" not in added  # off by default
        added = register.register(fft=False, rapsd=True)
        assert "utils.spectral:rapsd" in added and ref_mod.rapsd is spectral.rapsd
        assert ref_utils.interface.get_method("rapsd") is spectral.rapsd
        assert lookup("utils.spectral", "rapsd", spectral.rapsd) is original
        assert register.patch_rapsd() == []  # twice is once
    finally:
        register.unpatch_rapsd()
    assert ref_mod.rapsd is original and not hasattr(ref_mod, "_reference_rapsd")
    assert lookup("utils.spectral", "rapsd", spectral.rapsd) is original


def test_declined_shape_and_dtype_run_the_reference_for_every_method(ref_pysteps):
    """Shape and dtype are declined before the device is asked: through ``"hip"`` - no object the reference could call -
    the reference runs with ``np.fft``, its default method; so do ``rapsd_table`` with its default and the accumulator."""
    import warnings

    from pysteps.utils import spectral as ref

    from pysteps_amd.utils import spectral

    reference = getattr(ref, "_reference_rapsd", ref.rapsd)
    integers = np.arange(48 * 48, dtype=np.int32).reshape(48, 48) % 7
    long_side = restated.rain_field(5000, 64, 6).astype(np.float64)
    for field, why in ((integers, "a field of dtype int32"), (long_side, r"the shape \(5000, 64\)")):
        want, want_freq = reference(field, fft_method=np.fft, return_freq=True, d=3.0)
        for method in ("hip", np.fft):
            with pytest.warns(RuntimeWarning, match="pysteps_amd rapsd: %s - running the reference's function" % why):
                got, freq = spectral.rapsd(field, fft_method=method, return_freq=True, d=3.0)
            np.testing.assert_array_equal(got, want)
            np.testing.assert_array_equal(freq, want_freq)
        stack = np.stack([field, field[::-1].copy()])
        want_table = np.stack([want, reference(stack[1], fft_method=np.fft)])
        with pytest.warns(RuntimeWarning, match=why):
            np.testing.assert_array_equal(spectral.rapsd_table(stack), want_table)
        with pytest.warns(RuntimeWarning, match=why):
            acc = spectral.RapsdAccumulator(per_member=True, nan_value=0.0)
            acc(stack)
        np.testing.assert_array_equal(acc.member_spectra[0], want_table)
        np.testing.assert_array_equal(acc.mean_spectra[0], np.mean(want_table, axis=0))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            np.testing.assert_array_equal(spectral.rapsd(field, fft_method="hip", normalize=True),
                                          reference(field, fft_method=np.fft, normalize=True))
