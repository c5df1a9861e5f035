"""The Lagrangian probability nowcast on the device (``pysteps_amd.nowcasts.get_method("lagrangian_probability_hip")``,
csrc/lagprob.hip).

Held against tests/golden/lagprob_reference.npz (the unmodified reference's extrapolated stacks and outputs, written by
tools/make_golden_lagprob.py) and against the integer restatement of tests/helpers/lagprob.py, which
tests/test_lagprob_cpu.py holds to the reference.

* The probability stage is exact: the device counts the same two integers as the restatement and divides them in
  float64, so the comparison is bit for bit, NaN masks included.
* End to end the bar is 5 x the golden's ``fft_error`` (the reference's own FFT error against the exact counts), on
  every pixel.  The device extrapolator differs from the reference's by float32 rounding, and a pixel that changed
  sides of the threshold would change a count; every golden threshold sits ``gap`` away from the nearest extrapolated
  value, and the test first asserts that the device's extrapolated stack is within ``gap / 2`` of the stored one.
"""

import json
import os
import warnings

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import lagprob as restated

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "lagprob_reference.npz"))


def case_names():
    return [str(c) for c in np.load(os.path.join(GOLDEN, "lagprob_reference.npz"))["cases"]]


def load_case(golden, name):
    timesteps = json.loads(str(golden[name + "__timesteps"]))
    kwargs = json.loads(str(golden[name + "__kwargs"]))
    return (golden[name + "__precip"].astype(np.float64), golden[name + "__velocity"].astype(np.float64), timesteps,
            float(golden[name + "__threshold"]), kwargs)


def same_bits(got, want):
    """Equal as bit patterns apart from the NaN payload: same NaN mask, same float64 elsewhere (signed zeros too)."""
    if got.dtype != np.float64 or got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    return np.array_equal(got[ok].view(np.uint64), want[ok].view(np.uint64))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", case_names())
def test_stage_equals_restatement_on_golden_stacks(golden, name, dtype):
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.nowcasts.lagrangian_probability import probability_stage

    extrap = golden[name + "__extrap"].astype(dtype)
    threshold = float(golden[name + "__threshold"])
    scales = golden[name + "__scales"]
    got = probability_stage(DeviceArray.from_host(extrap), threshold, scales).to_host()
    want = restated.probability_stack(extrap, threshold, scales)
    assert same_bits(got, want)
    if dtype == np.float64:
        bar = 5.0 * float(golden["fft_error"])
        ref = golden[name + "__out"]
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        assert np.nanmax(np.abs(got - ref), initial=0.0) <= bar


def synthetic(m, n, seed):
    """Seeded field with wet cells of many sizes, a NaN wedge from a corner, a NaN block and scattered NaN pixels."""
    rng = np.random.default_rng(seed)
    coarse = rng.random((m // 24 + 2, n // 24 + 2))
    field = np.kron(coarse, np.ones((24, 24)))[:m, :n] + 0.3 * rng.random((m, n))
    field = field.astype(np.float32)
    yy, xx = np.mgrid[0:m, 0:n]
    field[yy + 2 * xx < n // 3] = np.nan
    field[m // 2 : m // 2 + 300, n // 3 : n // 3 + 280] = np.nan
    field[rng.random((m, n)) < 0.002] = np.nan
    return field


@pytest.mark.parametrize("shape", [(4096, 4096), (1226, 761), (640, 710)])
def test_stage_equals_restatement_on_large_fields(shape):
    """Scales 5, 60, 120 and 255 in one call.  The host restatement is computed for 40 output rows per plane: the
    first and last six rows of the image, the six rows around the upper edge of the NaN block, and 22 rows drawn
    with a seeded generator; every column of those rows is compared."""
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.nowcasts.lagrangian_probability import probability_stage

    m, n = shape
    scales = [5, 60, 120, 255]
    threshold = 0.75
    field = synthetic(m, n, seed=m + n)
    stack = np.stack([field, field[::-1].copy(), field[:, ::-1].copy(), field[::-1, ::-1].copy()])
    got = probability_stage(DeviceArray.from_host(stack), threshold, scales).to_host()
    assert got.dtype == np.float64 and got.shape == stack.shape
    assert np.array_equal(np.isnan(got), np.isnan(stack))
    rng = np.random.default_rng(7)
    edge = np.arange(m // 2 - 3, m // 2 + 3)
    rows = np.unique(np.concatenate([np.arange(6), np.arange(m - 6, m), edge, m - 1 - edge, rng.integers(0, m, size=22)]))
    for i, s in enumerate(scales):
        want = restated.probability(stack[i], threshold, s, rows=rows)
        assert same_bits(got[i][rows], want), "scale %d" % s
        finite = want[np.isfinite(want)]
        assert np.unique(finite).size > 10 and finite.max() - finite.min() > 0.1  # the case is not trivial


@pytest.mark.parametrize("name", case_names())
def test_end_to_end_against_the_reference(golden, name):
    from pysteps_amd import nowcasts
    from pysteps_amd.nowcasts import extrapolation

    precip, velocity, timesteps, threshold, kwargs = load_case(golden, name)
    want_extrap, want = golden[name + "__extrap"], golden[name + "__out"]
    gap = float(golden[name + "__gap"])
    bar = 5.0 * float(golden["fft_error"])

    got_extrap = extrapolation.forecast(precip.copy(), velocity.copy(), timesteps,
                                        kwargs.get("extrap_method", "semilagrangian"), kwargs.get("extrap_kwargs"))
    assert np.array_equal(np.isnan(got_extrap), np.isnan(want_extrap))
    ok = ~np.isnan(want_extrap)
    drift = float(np.max(np.abs(got_extrap[ok] - want_extrap[ok]))) if ok.any() else 0.0
    print("%s: device extrapolation within %.3g of the reference's, gap %.3g" % (name, drift, gap))
    assert drift <= gap / 2, "a pixel could change sides of the threshold"

    got = nowcasts.get_method("lagrangian_probability_hip")(precip.copy(), velocity.copy(), timesteps, threshold, **kwargs)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    err = float(np.nanmax(np.abs(got - want), initial=0.0))
    print("%s: max |device - reference| = %.3g (bar %.3g)" % (name, err, bar))
    assert err <= bar
    # and exactly the counts of the reference's own extrapolated stack
    assert same_bits(got, restated.probability_stack(want_extrap, threshold, golden[name + "__scales"]))


def test_inputs_are_not_modified(golden):
    from pysteps_amd import nowcasts

    precip, velocity, timesteps, threshold, kwargs = load_case(golden, "nan_input_64x80")
    p0, v0 = precip.copy(), velocity.copy()
    nowcasts.get_method("lagrangian_probability_hip")(precip, velocity, timesteps, threshold, **kwargs)
    assert np.array_equal(precip, p0, equal_nan=True) and np.array_equal(velocity, v0)


@pytest.mark.parametrize("name", ["default_64x80", "nan_input_64x80", "float_list_53x75"])
def test_resident_form(golden, name):
    from pysteps_amd import nowcasts
    from pysteps_amd.device import DeviceArray

    fn = nowcasts.get_method("lagrangian_probability_hip")
    precip, velocity, timesteps, threshold, kwargs = load_case(golden, name)
    want = fn(precip, velocity, timesteps, threshold, **kwargs)
    for dtype in (np.float32, np.float64):
        got = fn(DeviceArray.from_host(precip.astype(dtype)), DeviceArray.from_host(velocity.astype(dtype)), timesteps,
                 threshold, **kwargs)
        assert isinstance(got, DeviceArray) and got.dtype == np.float64 and got.shape == want.shape
        assert same_bits(got.to_host(), want)
    with pytest.raises(ValueError, match="both be NumPy arrays or both be DeviceArrays"):
        fn(DeviceArray.from_host(precip.astype(np.float32)), velocity, timesteps, threshold)


def test_stage_rejects_what_the_kernels_do_not_take():
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.nowcasts.lagrangian_probability import probability_stage

    stack = DeviceArray.from_host(np.zeros((1, 8, 8), dtype=np.float32))
    with pytest.raises(NotImplementedError):
        probability_stage(stack, 0.5, [256])
    with pytest.raises(ValueError):
        probability_stage(stack, 0.5, [5, 5])


def test_pysteps_route(ref_pysteps, golden):
    from pysteps import nowcasts
    from pysteps.nowcasts import lagrangian_probability as ref

    from pysteps_amd import register
    from pysteps_amd.nowcasts import lagrangian_probability

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        register.register()
    fn = nowcasts.get_method("lagrangian_probability_hip")
    assert fn is lagrangian_probability.forecast
    assert nowcasts.get_method("lagrangian_probability") is ref.forecast
    precip, velocity, timesteps, threshold, kwargs = load_case(golden, "default_64x80")
    got = fn(precip, velocity, timesteps, threshold, **kwargs)
    assert np.nanmax(np.abs(got - golden["default_64x80__out"])) <= 5.0 * float(golden["fft_error"])


def test_delegation_returns_the_references_result(ref_pysteps, golden):
    from pysteps.nowcasts import lagrangian_probability as ref

    from pysteps_amd import nowcasts
    from pysteps_amd.device import DeviceArray

    fn = nowcasts.get_method("lagrangian_probability_hip")
    precip, velocity, _, threshold, _ = load_case(golden, "default_64x80")
    for kwargs, text in (({"extrap_method": "eulerian"}, "extrap_method='eulerian'"), ({"slope": 130}, "scale 260")):
        want = ref.forecast(precip.copy(), velocity.copy(), 2, threshold, **kwargs)
        with pytest.warns(UserWarning, match=text):
            got = fn(precip.copy(), velocity.copy(), 2, threshold, **kwargs)
        assert np.array_equal(got, want, equal_nan=True)
    with pytest.raises(NotImplementedError):
        fn(DeviceArray.from_host(precip.astype(np.float32)), DeviceArray.from_host(velocity.astype(np.float32)), 2,
           threshold, slope=130)
