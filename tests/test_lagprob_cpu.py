"""The Lagrangian probability nowcast's host side (no GPU): the integer yardstick against the reference's goldens, the
kernel span table, argument checks, registration.

Yardstick: tests/helpers/lagprob.py counts what the reference convolves.  Its distance to the reference's output is
the error of SciPy's FFT convolution, which tools/make_golden_lagprob.py measured over all cases and stored as
``fft_error``; the bar here and in tests/test_lagprob_gpu.py is 5 x that value (README: "regression bar at 5 x what it
showed").  Scales 0, 1 and 2 do not go through the FFT and are bit-equal.
"""

import inspect
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from helpers import lagprob as restated


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "lagprob_reference.npz"))


def case_names():
    return [str(c) for c in np.load(os.path.join(GOLDEN, "lagprob_reference.npz"))["cases"]]


def test_golden_covers_the_required_scales(golden):
    scales = set()
    for name in golden["cases"]:
        scales.update(int(s) for s in golden[str(name) + "__scales"])
    assert {0, 1, 2, 3, 4, 5, 6, 7, 10, 15, 60, 61} <= scales and max(scales) > 64
    assert 0.0 < float(golden["fft_error"]) <= 1e-6


@pytest.mark.parametrize("name", case_names())
def test_restatement_reproduces_the_reference(golden, name):
    bar = 5.0 * float(golden["fft_error"])
    extrap, want = golden[name + "__extrap"], golden[name + "__out"]
    scales = golden[name + "__scales"]
    got = restated.probability_stack(extrap, float(golden[name + "__threshold"]), scales)
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(np.isnan(want), np.isnan(extrap))
    for i, s in enumerate(scales):
        ok = ~np.isnan(want[i])
        err = float(np.max(np.abs(got[i][ok] - want[i][ok]))) if ok.any() else 0.0
        print("%s scale %d: max |restated - reference| = %.3g (bar %.3g)" % (name, s, err, bar))
        if s <= 2:
            assert np.array_equal(got[i], want[i], equal_nan=True)
        assert err <= bar


@pytest.mark.parametrize("scale", [1, 2, 3, 4, 5, 6, 9, 16, 31])
def test_restatement_equals_direct_convolution(scale):
    """The yardstick itself against SciPy's direct (exact on 0/1 data) convolution, even and odd scales."""
    from scipy.signal import convolve

    rng = np.random.default_rng(scale)
    a = rng.random((37, 45)) < 0.4
    k = restated.get_kernel(scale)
    want = convolve(a.astype(np.float64), k.astype(np.float64), mode="same", method="direct")
    assert np.array_equal(restated.neighbourhood_counts(a, k), np.rint(want).astype(np.int64))
    assert np.array_equal(np.rint(want), want)
    rows = np.array([0, 5, 36])
    assert np.array_equal(restated.neighbourhood_counts(a, k, rows), np.rint(want[rows]).astype(np.int64))


def test_span_table_is_the_flipped_centred_kernel():
    from pysteps_amd.nowcasts.lagrangian_probability import MAX_SCALE, kernel_spans

    assert MAX_SCALE == 255
    for scale in range(1, MAX_SCALE + 1):
        # the expected support from the formula: ones below 5, else the disc around scale // 2; entry (i, j) of the
        # kernel meets input offset (c - i, c - j), c = (scale - 1) // 2
        mid = scale // 2
        ii, jj = np.mgrid[:scale, :scale]
        kernel = np.ones((scale, scale), dtype=bool) if scale < 5 else (ii - mid) ** 2 + (jj - mid) ** 2 <= mid**2
        c = (scale - 1) // 2
        want = set(zip((c - ii[kernel]).tolist(), (c - jj[kernel]).tolist()))
        dy, lo, hi = kernel_spans(scale)
        assert dy.dtype == lo.dtype == hi.dtype == np.int32 and len(dy) == len(lo) == len(hi) == scale
        assert np.array_equal(dy, np.arange(scale) + c - scale + 1)
        got = set((int(y), x) for y, a, b in zip(dy, lo, hi) for x in range(int(a), int(b) + 1))
        assert got == want, scale
        assert len(got) == int((hi - lo + 1).sum())
        # what the C entry point requires of a table
        assert np.all(lo >= c - scale) and np.all(lo <= hi + 1) and np.all(hi <= c)
    # the even disc is not symmetric: the flip is observable
    assert restated.support_of(restated.get_kernel(6)) != {(-y, -x) for y, x in restated.support_of(restated.get_kernel(6))}


def test_signature_equals_the_reference(golden):
    from pysteps_amd.nowcasts.lagrangian_probability import forecast

    assert str(inspect.signature(forecast)) == str(golden["signature"])


def test_package_table():
    from pysteps_amd import nowcasts
    from pysteps_amd.nowcasts import lagrangian_probability

    assert nowcasts.get_method("lagrangian_probability_hip") is lagrangian_probability.forecast
    assert nowcasts.get_method("LAGRANGIAN_PROBABILITY_HIP") is lagrangian_probability.forecast
    with pytest.raises(ValueError):
        nowcasts.get_method("lagrangian_probability")


@pytest.fixture
def no_device(monkeypatch):
    """Any use of the HIP library fails the test: the checks must come first."""
    from pysteps_amd import _lib

    def refuse():
        raise AssertionError("the device was used before the argument checks")

    monkeypatch.setattr(_lib, "lib", refuse)


_TIMESTEPS = {"float": 2.5, "tuple": (1, 2), "zero": 0, "negative": -3, "none": None}


def test_timesteps_errors_as_recorded(golden, no_device):
    from pysteps_amd.nowcasts.lagrangian_probability import forecast

    errors = json.loads(str(golden["errors"]))
    assert {e["label"] for e in errors} == set(_TIMESTEPS)
    p, v = np.ones((16, 16)), np.zeros((2, 16, 16))
    for e in errors:
        assert e["type"] == "ValueError"
        with pytest.raises(ValueError) as err:
            forecast(p, v, _TIMESTEPS[e["label"]], 1.0)
        assert str(err.value) == e["message"], e["label"]


def _bad_inputs():
    return [
        ((np.zeros((4, 16, 16)), np.zeros((2, 16, 16)), 3, 1.0), "The input precipitation must be a two-dimensional array"),
        ((np.zeros((16, 16)), np.zeros((16, 16)), 3, 1.0), "Input velocity must be a three-dimensional array"),
        ((np.zeros((16, 16)), np.zeros((2, 16, 17)), 3, 1.0),
         "Dimension mismatch between input precipitation and velocity: shape(precip)=(16, 16), shape(velocity)=(2, 16, 17)"),
        ((np.zeros((16, 16)), np.zeros((2, 16, 16)), [2, 1], 1.0), "timesteps is not in ascending order"),
        ((np.zeros((16, 16)), np.full((2, 16, 16), np.nan), 3, 1.0), "velocity contains non-finite values"),
        ((np.full((16, 16), np.nan), np.zeros((2, 16, 16)), 3, 1.0), "precip contains only non-finite values"),
    ]


@pytest.mark.parametrize("args,message", _bad_inputs())
def test_input_errors_before_device(no_device, args, message):
    from pysteps_amd.nowcasts.lagrangian_probability import forecast

    with pytest.raises(ValueError) as err:
        forecast(*args)
    assert str(err.value) == message


@pytest.mark.parametrize("args,message", _bad_inputs())
def test_input_errors_match_reference(ref_pysteps, args, message):
    from pysteps.nowcasts import lagrangian_probability as ref

    with pytest.raises(ValueError) as err:
        ref.forecast(*args)
    assert str(err.value) == message


def test_delegation_without_device(ref_pysteps, no_device):
    """Another extrapolation method and a scale above 255 go to the reference, with a warning."""
    from pysteps.nowcasts import lagrangian_probability as ref

    from pysteps_amd.nowcasts.lagrangian_probability import forecast

    rng = np.random.default_rng(5)
    p = np.round(rng.random((40, 48)) * 40.0) / 4.0
    v = np.full((2, 40, 48), 0.5)
    want = ref.forecast(p.copy(), v.copy(), 2, 2.5, extrap_method="eulerian")
    with pytest.warns(UserWarning, match="extrap_method='eulerian'"):
        got = forecast(p.copy(), v.copy(), 2, 2.5, extrap_method="eulerian")
    assert np.array_equal(got, want, equal_nan=True)
    want = ref.forecast(p.copy(), v.copy(), [1], 2.5, slope=256)
    with pytest.warns(UserWarning, match="scale 256"):
        got = forecast(p.copy(), v.copy(), [1], 2.5, slope=256)
    assert np.array_equal(got, want, equal_nan=True)


def test_register_adds_lagrangian_probability_hip(ref_pysteps):
    from pysteps import nowcasts
    from pysteps.nowcasts import lagrangian_probability as ref

    from pysteps_amd import register
    from pysteps_amd.nowcasts import lagrangian_probability

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        added = register.register()
    assert "nowcast:lagrangian_probability_hip" in added and "nowcast:anvil_hip" in added
    assert nowcasts.get_method("lagrangian_probability_hip") is lagrangian_probability.forecast
    assert nowcasts.get_method("lagrangian_probability") is ref.forecast
    assert ref.forecast is not lagrangian_probability.forecast


def test_imports_without_pysteps_and_without_gpu():
    code = (
        "import sys\n"
        "class Block:\n"
        "    def find_spec(self, name, path=None, target=None):\n"
        "        if name == 'pysteps' or name.startswith('pysteps.'):\n"
        "            raise ImportError('pysteps is blocked in this test')\n"
        "sys.meta_path.insert(0, Block())\n"
        "import pysteps_amd.nowcasts.lagrangian_probability as lp\n"
        "from pysteps_amd import nowcasts\n"
        "assert nowcasts.get_method('lagrangian_probability_hip') is lp.forecast\n"
        "assert lp.kernel_spans(5)[1].tolist() == [0, -1, -2, -1, 0]\n"
        "assert not any(k == 'pysteps' or k.startswith('pysteps.') for k in sys.modules)\n"
        "print('ok')\n"
    )
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stderr
