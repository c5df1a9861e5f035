"""The ANVIL nowcast's host side (no GPU): band-pass weights, argument checks, delegation, registration."""

import contextlib
import io
import os
import warnings

import numpy as np
import pytest

from conftest import GOLDEN


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "anvil_reference.npz"))


@pytest.mark.parametrize("tag,shape,levels", [("bp_64x48", (64, 48), 6), ("bp_75x101", (75, 101), 5)])
def test_filter_gaussian_matches_reference_weights(golden, tag, shape, levels):
    from pysteps_amd.cascade.bandpass_filters import filter_gaussian

    bp = filter_gaussian(shape, levels)
    assert np.array_equal(bp["weights_1d"], golden[tag + "__w1"])
    assert np.array_equal(bp["weights_2d"], golden[tag + "__w2"])
    assert bp["shape"] == shape and len(bp["central_wavenumbers"]) == levels
    with pytest.raises(ValueError, match="n must be greater than 2"):
        filter_gaussian(shape, 2)


@pytest.fixture
def no_device(monkeypatch):
    """Any use of the HIP library fails the test: the checks must come first."""
    from pysteps_amd import _lib

    def refuse():
        raise AssertionError("the device was used before the argument checks")

    monkeypatch.setattr(_lib, "lib", refuse)


def _bad_calls():
    v4 = np.zeros((4, 16, 16))
    vel = np.zeros((2, 16, 16))
    return [
        ((np.zeros((16, 16)), vel, 3), {}, "vil.shape = (16, 16), but a three-dimensional array expected"),
        ((v4, vel, 3), {"rainrate": np.zeros(16)}, "rainrate.shape = (16,), but a two-dimensional array expected"),
        ((v4, vel, 3), {"ar_order": 1}, "vil.shape[0] = 4, but vil.shape[0] = ar_order + 2 = 3 required"),
        ((v4, np.zeros((16, 16)), 3), {}, "velocity.shape = (16, 16), but a three-dimensional array expected"),
        ((v4, vel, [2, 1]), {}, "timesteps is not in ascending order"),
    ]


@pytest.mark.parametrize("args,kwargs,message", _bad_calls())
def test_argument_errors_before_device(no_device, args, kwargs, message):
    from pysteps_amd.nowcasts.anvil import forecast

    with pytest.raises(ValueError) as err:
        forecast(*args, **kwargs)
    assert str(err.value) == message


@pytest.mark.parametrize("args,kwargs,message", _bad_calls())
def test_argument_errors_match_reference(ref_pysteps, args, kwargs, message):
    from pysteps.nowcasts import anvil as ref

    with pytest.raises(ValueError) as err:
        ref.forecast(*args, **kwargs)
    assert str(err.value) == message


def test_ar_order_3_delegates(ref_pysteps, no_device):
    from pysteps.nowcasts import anvil as ref

    from pysteps_amd.nowcasts.anvil import forecast

    rng = np.random.default_rng(3)
    vil = np.maximum(rng.standard_normal((5, 32, 32)) * 5.0 + 5.0, 0.0)
    vel = np.full((2, 32, 32), 0.5)
    kw = dict(timesteps=2, ar_order=3, ar_window_radius=5)
    with contextlib.redirect_stdout(io.StringIO()):
        want = ref.forecast(vil.copy(), vel.copy(), **kw)
        with pytest.warns(UserWarning, match="ar_order=3"):
            got = forecast(vil.copy(), vel.copy(), **kw)
    assert np.array_equal(got, want, equal_nan=True)


def test_register_adds_anvil_hip(ref_pysteps):
    from pysteps import nowcasts

    from pysteps_amd import register
    from pysteps_amd.nowcasts import anvil

    stock = nowcasts.get_method("anvil")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        added = register.register()
    assert "nowcast:anvil_hip" in added
    assert nowcasts.get_method("anvil_hip") is anvil.forecast
    assert nowcasts.get_method("anvil") is stock and stock is not anvil.forecast


def test_package_table():
    from pysteps_amd import nowcasts
    from pysteps_amd.nowcasts import anvil

    assert nowcasts.get_method("anvil_hip") is anvil.forecast
    with pytest.raises(ValueError):
        nowcasts.get_method("anvil_cpu")
