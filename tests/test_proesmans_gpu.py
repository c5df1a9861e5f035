"""The Proesmans motion estimate on the device (``pysteps_amd.motion.get_method("proesmans_hip")``, csrc/proesmans.hip).

Stages are held bit for bit to the float64 restatement of tests/helpers/proesmans.py (itself equal to the compiled
reference bit for bit, test_proesmans_cpu.py) from a mid-run state with non-zero vectors: the device performs the same
IEEE operations in the same order, so identity is derived, not hoped for.  The one exception is ``c_sum``: the reference
adds in raster order, the device rounds the exact sum once - held within one unit in the last place of ``math.fsum``.

Whole calls are held, on the stored pixels of tests/golden/proesmans_reference.npz, bit for bit to the restatement
evaluated with the exact ``c_sum`` and, within 5 x the case's own deviation (proesmans_bars.json: the largest difference
between the unmodified reference and that restatement, at most 1e-8 by the tool's assertion), to the reference itself.
The sweep test and the whole calls fail for any implementation that does not keep the reference's update order: a sweep
from the old field alone moves the vectors by more than 1e-3 (asserted below for the sweep)."""

import json
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import proesmans as hp

pytestmark = pytest.mark.gpu

LAM = 50.0


def pm():
    from pysteps_amd.motion import proesmans as module

    return module


def dev(a):
    from pysteps_amd.device import DeviceArray

    return DeviceArray.from_host(np.ascontiguousarray(a))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "proesmans_reference.npz"))


@pytest.fixture(scope="module")
def bars():
    with open(os.path.join(GOLDEN, "proesmans_bars.json")) as f:
        return json.load(f)["own_deviation"]


def _device_cases():
    z = np.load(os.path.join(GOLDEN, "proesmans_reference.npz"))
    return [str(c) for c in z["cases"] if not str(c).startswith("cpu_")]


@pytest.fixture(scope="module")
def state():
    """A restated mid-run state on 150 x 131 (three 64-row blocks, two t-tiles): three iterations on the 75 x 65
    level, carried up."""
    frames = hp.recipe_frames(150, 131, 7)
    scaled = hp.scale_frames(frames)
    pyr = [hp.pyramid(scaled[0], 3), hp.pyramid(scaled[1], 3)]
    R1 = np.stack([pyr[0][1], pyr[1][1]])
    G1 = np.stack([hp.gradients(R1[0]), hp.gradients(R1[1])])
    V1 = np.zeros((2, 2, 75, 65))
    for _ in range(3):
        hp.sweep(V1, hp.consistency_maps(V1, "exact"), R1, G1, LAM)
    V0 = hp.next_level(V1, 150, 131)
    assert np.max(np.abs(V0)) > 0.5
    R0 = np.stack([pyr[0][0], pyr[1][0]])
    G0 = np.stack([hp.gradients(R0[0]), hp.gradients(R0[1])])
    return dict(frames=frames, scaled=scaled, pyr=pyr, V1=V1, V0=V0, R0=R0, G0=G0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_scale_bit_for_bit(state, dtype):
    frames = state["frames"].astype(dtype)
    got, (lo, hi, bad) = pm().scale_frames(dev(frames))
    assert (lo, hi, bad) == (float(frames.min()), float(frames.max()), 0)
    assert np.array_equal(got.to_host(), hp.scale_frames(frames))
    flat = np.full((2, 5, 7), 3.25, dtype)
    assert np.array_equal(pm().scale_frames(dev(flat))[0].to_host(), flat.astype(np.float64))  # max - min <= 1e-8
    flat[1, 2, 3] = np.nan
    flat[0, 0, 0] = np.inf
    assert pm().scale_frames(dev(flat))[1][2] == 2


def test_pyramid_bit_for_bit(state):
    level = dev(state["scaled"][1])
    for want in state["pyr"][1][1:]:  # 150 x 131 -> 75 x 65 -> 37 x 32: odd last row and column dropped
        level = pm().pyramid_level(level)
        assert level.shape == want.shape and np.array_equal(level.to_host(), want)


@pytest.mark.parametrize("level", [0, 2])
def test_gradients_bit_for_bit(state, level):
    I = state["pyr"][0][level]
    assert np.array_equal(pm().gradients(dev(I)).to_host(), hp.gradients(I))


def test_consistency_stages(state):
    V = state["V0"]
    gamma, raw, stats = pm().consistency_maps(dev(V), stages=True)
    raw, stats = raw.to_host(), stats.to_host()
    want_raw = hp.consistency_raw(V)
    assert np.count_nonzero(want_raw < 0) > 0, "no displaced pixel leaves the image: the -1 branch is not covered"
    assert np.array_equal(raw, want_raw)
    for i in range(2):
        exact, count = hp.consistency_sum(want_raw[i], "exact")
        assert stats[i, 1] == count
        assert abs(stats[i, 0] - exact) <= np.spacing(exact), (stats[i, 0], exact)
        assert stats[i, 2] == 0.9 * stats[i, 0] / count and stats[i, 2] > 1e-8
        assert np.array_equal(gamma.to_host()[i], hp.consistency_normalise(want_raw[i], stats[i, 2]))


def test_consistency_of_a_zero_field_is_one():
    """K = 0 <= 1e-8: every value is 1."""
    gamma, raw, stats = pm().consistency_maps(dev(np.zeros((2, 2, 9, 70))), stages=True)
    assert np.array_equal(gamma.to_host(), np.ones((2, 9, 70))) and np.array_equal(raw.to_host(), np.zeros((2, 9, 70)))
    assert np.array_equal(stats.to_host()[:, :3], [[0.0, 630.0, 0.0]] * 2)


def _random_state(m, n, seed):
    rng = np.random.default_rng(seed)
    R = rng.random((2, m, n)) * 255.0
    G = np.stack([hp.gradients(R[0]), hp.gradients(R[1])])
    V = rng.standard_normal((2, 2, m, n)) * 1.5
    GAMMA = rng.random((2, m, n))
    GAMMA[rng.random((2, m, n)) < 0.3] = 0.0  # patches whose weights sum below 1e-8
    GAMMA[:, 5:12, 20:40] = 0.0
    return V, GAMMA, R, G


def _sweep_states(state):
    yield "mid-run 150 x 131", state["V0"], hp.consistency_maps(state["V0"], "exact"), state["R0"], state["G0"]
    # two row blocks and four t-tiles; five row blocks and one t-tile; a single interior pixel
    for m, n in ((70, 300), (259, 5), (3, 3)):
        yield ("random %d x %d" % (m, n),) + _random_state(m, n, m + n)


def test_sweep_bit_for_bit(state):
    """One sweep plus edge fill from the same V, GAMMA, frames and gradients, both directions."""
    for label, V, GAMMA, R, G in _sweep_states(state):
        want = V.copy()
        hp.sweep(want, GAMMA, R, G, LAM)
        got = dev(V)
        pm().sweep(got, dev(GAMMA), dev(R), dev(G), LAM)
        assert np.array_equal(got.to_host(), want), label
        if V.shape[2] > 3:
            other = V.copy()
            hp.sweep_jacobi(other, GAMMA, R, G, LAM)
            assert np.max(np.abs(other - want)) > 1e-3, label  # the order matters on this state


def test_next_level_bit_for_bit(state):
    V1 = state["V1"]
    got = pm().next_level(dev(V1), 150, 131)  # column 130 copies the clamped index 64
    assert np.array_equal(got.to_host(), state["V0"])
    small = V1[:, :, :37, :32]
    got = pm().next_level(dev(small), 75, 65)  # row 74 and column 64 clamp
    assert np.array_equal(got.to_host(), hp.next_level(small, 75, 65))


@pytest.mark.parametrize("name", _device_cases())
def test_whole_call(golden, bars, name):
    c = hp.golden_case(golden, name)
    s = c["stride"]
    V, G = pm().proesmans(c["frames"], full_output=True, **c["kw"])
    assert V.dtype == np.float64 and V.shape == (2, 2) + c["frames"].shape[1:] and G.shape == (2,) + c["frames"].shape[1:]
    V, G = V[..., ::s, ::s], G[..., ::s, ::s]
    to_ref = (float(np.max(np.abs(V - c["ref_V"]))), float(np.max(np.abs(G - c["ref_G"]))))
    to_exact = (float(np.max(np.abs(V - c["exact_V"]))), float(np.max(np.abs(G - c["exact_G"]))))
    print("%s: to the reference V %.3e GAMMA %.3e (own deviation %.3e, %.3e); to the exact restatement %.3e %.3e"
          % (name, to_ref[0], to_ref[1], bars[name]["V"], bars[name]["GAMMA"], to_exact[0], to_exact[1]))
    assert np.array_equal(V, c["exact_V"]) and np.array_equal(G, c["exact_G"]), to_exact
    assert to_ref[0] <= 5.0 * bars[name]["V"] and to_ref[1] <= 5.0 * bars[name]["GAMMA"], to_ref


def test_outputs_and_residency(golden):
    """full_output=False is advfield[0]; two runs give the same bits; float32 resident frames give float32 resident
    fields equal to the float64 result rounded once, and feed semilagrangian_hip as they are."""
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.extrapolation import get_method

    c = hp.golden_case(golden, "d150x131_l3_i10_f32")
    frames = c["frames"]
    assert frames.dtype == np.float32
    V, G = pm().proesmans(frames, full_output=True, **c["kw"])  # a float32 host array is widened
    again = pm().proesmans(frames, full_output=True, **c["kw"])
    assert np.array_equal(again[0], V) and np.array_equal(again[1], G)
    assert np.array_equal(pm().proesmans(frames, **c["kw"]), V[0])
    stats = pm().last_run_stats
    assert stats["launches_per_iteration"] == pm().launches_per_iteration(150, 131) > 4 and stats["total"] > 0.0

    Vd, Gd = pm().proesmans(dev(frames), full_output=True, **c["kw"])
    assert isinstance(Vd, DeviceArray) and Vd.dtype == np.float32 and Gd.dtype == np.float32
    assert np.array_equal(Vd.to_host(), V.astype(np.float32)) and np.array_equal(Gd.to_host(), G.astype(np.float32))
    V64 = pm().proesmans(dev(frames.astype(np.float64)), full_output=True, **c["kw"])[0]
    assert V64.dtype == np.float64 and np.array_equal(V64.to_host(), V)

    field = pm().proesmans(dev(frames), **c["kw"])
    assert isinstance(field, DeviceArray) and field.shape == (2, 150, 131) and field.dtype == np.float32
    precip = frames[1]
    out = get_method("semilagrangian_hip")(dev(precip), field, 2)
    want = get_method("semilagrangian_hip")(dev(precip), dev(V[0].astype(np.float32)), 2)
    assert isinstance(out, DeviceArray) and out.shape == (2, 150, 131)
    assert np.array_equal(out.to_host(), want.to_host(), equal_nan=True)


def test_filter_std_equals_prefiltered_frames(state):
    from scipy.ndimage import gaussian_filter

    V, G = pm().proesmans(state["frames"], num_iter=4, num_levels=3, filter_std=1.0, full_output=True)
    im = state["scaled"].copy()
    im[0], im[1] = gaussian_filter(im[0], 1.0), gaussian_filter(im[1], 1.0)
    Vp, Gp = pm().advection_field(dev(im), LAM, 4, 3)
    assert np.array_equal(V, Vp.to_host()) and np.array_equal(G, Gp.to_host())
    plain = pm().proesmans(state["frames"], num_iter=4, num_levels=3, full_output=True)[0]
    assert not np.array_equal(plain, V)


def test_resident_non_finite_frames_go_to_the_reference(ref_pysteps):
    frames = hp.recipe_frames(48, 40, 2)
    frames[0, 3, 3] = np.inf
    with pytest.warns(RuntimeWarning, match="non-finite input"):
        got = pm().proesmans(dev(frames), num_iter=2, num_levels=2)
    assert got.shape == (2, 48, 40)


def test_c_sum_is_the_exact_sum_on_a_hard_plane():
    """Values spread over 30 orders of magnitude: a plain sum in any order loses what the double-double keeps."""
    m, n = 40, 90
    rng = np.random.default_rng(11)
    V = np.zeros((2, 2, m, n))
    V[0, 0] = 10.0 ** rng.uniform(-20, -1, (m, n))  # c = |u + ub| with the backward field zero
    V[1, 1] = -(10.0 ** rng.uniform(-25, -2, (m, n)))
    _, raw, stats = pm().consistency_maps(dev(V), stages=True)
    want_raw = hp.consistency_raw(V)
    assert np.array_equal(raw.to_host(), want_raw)
    for i in range(2):
        exact, count = hp.consistency_sum(want_raw[i], "exact")
        got = stats.to_host()[i]
        assert got[1] == count and abs(got[0] - exact) <= np.spacing(exact)
        assert math.isfinite(got[2])
