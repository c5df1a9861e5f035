"""The Proesmans motion estimate's host side (no GPU): the stage-by-stage restatement (tests/helpers/proesmans.py) held
to the goldens of the unmodified reference (tests/golden/proesmans_reference.npz, tools/make_golden_proesmans.py),
registration, the argument checks and what leaves the device path.  test_proesmans_gpu.py holds the device to the
restatement."""

import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import proesmans as hp

SMALL = ("cpu_41x37_l2_i4", "cpu_70x33_l3_i3")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "proesmans_reference.npz"))


@pytest.fixture
def no_device(monkeypatch):
    """Any use of the HIP library fails the test: the checks and the delegation decision come first."""
    from pysteps_amd import _lib

    def refuse():
        raise AssertionError("the device was used")

    monkeypatch.setattr(_lib, "lib", refuse)


@pytest.mark.parametrize("name", SMALL)
def test_restatement_equals_the_reference_bit_for_bit(golden, name):
    c = hp.golden_case(golden, name)
    assert c["stride"] == 1
    V, G = hp.proesmans(c["frames"], full_output=True, c_sum="sequential", **c["kw"])
    assert np.array_equal(V, c["ref_V"]) and np.array_equal(G, c["ref_G"])
    assert np.max(np.abs(c["ref_V"])) > 1.0  # the fields are not trivial


@pytest.mark.parametrize("name", SMALL)
def test_exact_sum_restatement_equals_the_stored_one(golden, name):
    c = hp.golden_case(golden, name)
    V, G = hp.proesmans(c["frames"], full_output=True, c_sum="exact", **c["kw"])
    assert np.array_equal(V, c["exact_V"]) and np.array_equal(G, c["exact_G"])


@pytest.mark.parametrize("name", SMALL)
def test_jacobi_sweep_misses_the_goldens(golden, name):
    """A sweep from the old field alone is another algorithm, and the goldens tell."""
    c = hp.golden_case(golden, name)
    V, _ = hp.proesmans(c["frames"], full_output=True, jacobi=True, **c["kw"])
    assert np.max(np.abs(V - c["ref_V"])) > 1e-3


def test_bars_hold_the_cap(golden):
    """Every device case's own deviation (reference against the exactly summed restatement) is at most 1e-8."""
    with open(os.path.join(GOLDEN, "proesmans_bars.json")) as f:
        bars = json.load(f)
    names = [str(c) for c in golden["cases"]]
    device = [n for n in names if n not in SMALL]
    assert len(device) >= 7 and set(bars["own_deviation"]) == set(names)
    for n in device:
        assert 0.0 <= bars["own_deviation"][n]["V"] <= 1e-8 and 0.0 <= bars["own_deviation"][n]["GAMMA"] <= 1e-8, n


def test_gradient_restatement_equals_scipy():
    from scipy.ndimage import convolve

    rng = np.random.default_rng(3)
    for shape in ((37, 41), (3, 3), (1, 5), (64, 2)):
        I = rng.random(shape) * 255.0
        I[rng.random(shape) < 0.2] = 0.0
        got = hp.gradients(I)
        for k, K in enumerate(hp.gradient_kernels()):
            assert np.array_equal(got[k], convolve(I, K, mode="constant", cval=0.0)), (shape, k)


def test_package_table():
    from pysteps_amd import motion
    from pysteps_amd.motion.proesmans import proesmans

    assert motion.get_method("proesmans_hip") is proesmans
    assert motion.get_method("Proesmans_HIP") is proesmans


def test_register_into_adds_proesmans_hip():
    from pysteps_amd import register
    from pysteps_amd.motion.proesmans import proesmans

    stock = object()
    for override in (False, True):
        motion = {"proesmans": stock}
        added = register.register_into(motion, None, override=override)
        assert "motion:proesmans_hip" in added
        assert motion["proesmans_hip"] is proesmans and motion["proesmans"] is stock


def test_pysteps_tables(ref_pysteps):
    import pysteps.motion as ref_motion
    import pysteps.motion.interface as mot_if

    from pysteps_amd import motion, register
    from pysteps_amd.motion.proesmans import proesmans

    stock = ref_motion.get_method("proesmans")
    assert stock is not proesmans and motion.get_method("proesmans") is stock
    saved = dict(mot_if._methods)
    try:
        register.register_into(mot_if._methods, None)
        assert ref_motion.get_method("proesmans_hip") is proesmans
        assert ref_motion.get_method("proesmans") is stock and motion.get_method("proesmans") is stock
    finally:
        mot_if._methods.clear()
        mot_if._methods.update(saved)


@pytest.mark.parametrize("frames", [np.zeros((40, 40)), np.zeros((3, 40, 40)), np.zeros((1, 2, 40, 40))])
def test_argument_checks_raise_the_reference_messages(no_device, ref_pysteps, frames):
    from pysteps.motion.proesmans import proesmans as ref

    from pysteps_amd.motion.proesmans import proesmans

    with pytest.raises(ValueError) as want:
        ref(frames)
    with pytest.raises(ValueError) as got:
        proesmans(frames)
    assert str(got.value) == str(want.value)


def test_one_frame_raises_as_the_reference(no_device, ref_pysteps):
    from pysteps.motion.proesmans import proesmans as ref

    from pysteps_amd.motion.proesmans import proesmans

    with pytest.raises(IndexError) as want:
        ref(np.zeros((1, 40, 40)))
    with pytest.raises(IndexError) as got:
        proesmans(np.zeros((1, 40, 40)))
    assert str(got.value) == str(want.value)


def test_small_coarsest_level_goes_to_the_reference(no_device, ref_pysteps):
    from pysteps.motion.proesmans import proesmans as ref

    from pysteps_amd.motion.proesmans import proesmans

    frames = hp.recipe_frames(40, 70, 2)  # 6 levels: the coarsest is 1 x 2
    want = ref(frames.copy(), num_iter=3, full_output=True)
    with pytest.warns(RuntimeWarning, match="coarsest pyramid level of 1 x 2"):
        got = proesmans(frames.copy(), num_iter=3, full_output=True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_non_finite_input_goes_to_the_reference(no_device, ref_pysteps):
    from pysteps.motion.proesmans import proesmans as ref

    from pysteps_amd.motion.proesmans import proesmans

    frames = hp.recipe_frames(48, 40, 2)
    frames[1, 7, 9] = np.nan
    want = ref(frames.copy(), num_iter=2, num_levels=2)
    with pytest.warns(RuntimeWarning, match="non-finite input"):
        got = proesmans(frames.copy(), num_iter=2, num_levels=2)
    assert got.shape == want.shape == (2, 48, 40) and np.array_equal(got, want, equal_nan=True)


def test_declined_without_pysteps_raises(no_device, monkeypatch):
    from pysteps_amd.motion import proesmans as pm

    monkeypatch.setattr(pm, "lookup", lambda module, name, ours: None)
    with pytest.raises(NotImplementedError, match="coarsest pyramid level"):
        pm.proesmans(np.zeros((2, 40, 70)))
    bad = np.zeros((2, 128, 128))
    bad[0, 0, 0] = np.inf
    with pytest.raises(NotImplementedError, match="non-finite"):
        pm.proesmans(bad)


def test_supported_shapes_reach_the_device(monkeypatch):
    """The smallest shape the defaults take: 96 x 96 halves five times to 3 x 3."""
    from pysteps_amd.motion import proesmans as pm

    assert pm._unsupported((2, 96, 96), 6) is None and pm._unsupported((2, 95, 96), 6) is not None
    assert pm._unsupported((2, 3, 3), 1) is None and pm._unsupported((2, 2, 3), 1) is not None
