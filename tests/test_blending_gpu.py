"""Linear and salient blending on the device (``pysteps_amd.blending``, csrc/blending.hip).

The blend is made of correctly rounded IEEE operations and integer ranks only, so the device is held to the goldens of
the unmodified reference (tests/golden/blending_reference.npz) with no tolerance: ``np.array_equal`` on NaN-free
results, for host and resident inputs.  The whole call is held bit for bit to the helper's restatement applied to the
device's own nowcast.  The one transcendental is the float64 dB inverse: held to 5 x the reference's own deviation from
a long-double restatement (blending_bars.json, in units in the last place), the project's standing margin for a second
correctly implemented ``pow``."""

import ctypes
import json
import os
import warnings

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import blending as hb

pytestmark = pytest.mark.gpu

RATE_META = {"transform": None, "unit": "mm/h", "threshold": 0.1, "zerovalue": 0.0}


def lb():
    from pysteps_amd.blending import linear_blending as module

    return module


def dev(a):
    from pysteps_amd.device import DeviceArray

    return DeviceArray.from_host(np.ascontiguousarray(a))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "blending_reference.npz"))


@pytest.fixture(scope="module")
def bars():
    with open(os.path.join(GOLDEN, "blending_bars.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("resident", [False, True], ids=["host", "resident"])
@pytest.mark.parametrize("saliency", [False, True], ids=["linear", "salient"])
@pytest.mark.parametrize("name", sorted(hb.CASES))
def test_blend_equals_reference_bit_for_bit(golden, name, saliency, resident):
    from pysteps_amd.device import DeviceArray

    nowcast, nwp, kwargs = hb.make_case(name)
    assert hb.digest(nowcast, nwp) == str(golden[name + "__sha256"])
    want = golden[name + ("__salient" if saliency else "__linear")]
    before = nowcast.copy(), nwp.copy()
    if resident:
        d_nowcast, d_nwp = dev(nowcast), dev(nwp)
        got = lb().blend(d_nowcast, d_nwp, saliency=saliency, **kwargs)
        assert isinstance(got, DeviceArray)
        got = got.to_host()
        assert np.array_equal(d_nowcast.to_host(), nowcast, equal_nan=True) and np.array_equal(d_nwp.to_host(), nwp, equal_nan=True)
    else:
        got = lb().blend(nowcast, nwp, saliency=saliency, **kwargs)
        assert isinstance(got, np.ndarray)
    assert np.array_equal(nowcast, before[0], equal_nan=True) and np.array_equal(nwp, before[1], equal_nan=True)
    assert got.shape == want.shape and got.dtype == want.dtype
    assert not np.isnan(want).any()
    differ = np.count_nonzero(got != want)
    print("%s %s: %d of %d values differ" % (name, "salient" if saliency else "linear", differ, want.size))
    assert np.array_equal(got, want)


def _dense_rank(x):
    from pysteps_amd import _lib
    from pysteps_amd.device import DeviceArray

    d_x = dev(x)
    rank = DeviceArray(x.shape, np.uint32)
    distinct = ctypes.c_uint(0)
    _lib.check(_lib.lib().psh_blend_dense_rank_dev(d_x.ptr, int(x.dtype == np.float32), x.size, rank.ptr, ctypes.byref(distinct)),
               "psh_blend_dense_rank_dev")
    return rank.to_host(), distinct.value


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", ["dry", "distinct", "equal", "signed", "single"])
def test_dense_rank_equals_np_unique(kind, dtype):
    """The ranking alone: 300 x 300 keys (44 tiles), more than 90 % of them one value; all distinct; all equal (every
    digit constant, no pass runs); both signs, -0.0 with 0.0, neighbours in the last bit, the extremes; one key."""
    rng = np.random.default_rng(5)
    n = 300 * 300
    if kind == "dry":
        x = np.where(rng.random(n) < 0.93, 0.0, np.round(rng.gamma(0.6, 4.0, n) * 8.0) / 8.0)
    elif kind == "distinct":
        x = rng.permutation(n) * 0.37 - 1e4
    elif kind == "equal":
        x = np.full(n, 2.5)
    elif kind == "signed":
        x = rng.standard_normal(n) * 1e3
        x[::7] = -0.0
        x[1::7] = 0.0
        x[2::7] = np.nextafter(dtype(1.0), dtype(2.0))
        x[3::7] = 1.0
        x[4::97] = np.finfo(dtype).max
        x[5::97] = -np.finfo(dtype).max
        x[6::97] = np.finfo(dtype).tiny
    else:
        x = np.array([3.0])
    x = x.astype(dtype)
    values, inverse = np.unique(x, return_inverse=True)
    rank, distinct = _dense_rank(x)
    assert distinct == len(values)
    assert np.array_equal(rank, (inverse + 1).astype(np.uint32))


def _whole_call_inputs():
    from tools import synth

    m, n = 96, 128
    frames = np.stack([synth.rain_field_db(m, n, seed=5), synth.rain_field_db(m, n, seed=5)]).astype(np.float32)
    velocity = synth.true_velocity(m, n)
    rng = np.random.default_rng(77)
    nwp = hb.rain(rng, (2, 6, m, n))
    nwp[0, 1, 3, 4] = np.nan
    meta = {"transform": "dB", "unit": "mm/h", "threshold": -10.0, "zerovalue": -15.0}
    return frames, velocity, nwp, meta


@pytest.mark.parametrize("saliency", [False, True], ids=["linear", "salient"])
def test_whole_call_equals_restatement_of_its_own_nowcast(saliency):
    """``forecast`` with the device's extrapolation nowcast, resident float32 dB frames and a host float64 NWP ensemble
    of two members: the result is the restatement's blend of the device's own converted nowcast, bit for bit."""
    from pysteps_amd.blending import get_method
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.nowcasts import get_method as nowcast_method

    frames, velocity, nwp, meta = _whole_call_inputs()
    sch = dict(timesteps=5, timestep=5, start_blending=5, end_blending=20)
    d_frames, d_velocity = dev(frames), dev(velocity)
    name = "salient_blending_hip" if saliency else "linear_blending_hip"
    got = get_method(name)(d_frames, meta, d_velocity, sch["timesteps"], sch["timestep"], "extrapolation", precip_nwp=nwp,
                           precip_nwp_metadata=RATE_META, start_blending=sch["start_blending"], end_blending=sch["end_blending"])
    assert isinstance(got, DeviceArray) and got.shape == (2, 5, 96, 128) and got.dtype == np.float64
    nowcast = nowcast_method("extrapolation")(d_frames.view(1), d_velocity, 4)
    rate = lb().to_rainrate(nowcast, meta).to_host()
    assert rate.dtype == np.float32 and np.isnan(rate).any() and np.nanmax(rate) > 1.0
    want = hb.blend(rate, nwp, saliency=saliency, **sch)
    assert np.array_equal(got.to_host(), want)
    assert np.array_equal(d_frames.to_host(), frames)
    # without NWP data the converted nowcast comes back
    alone = get_method(name)(d_frames, meta, d_velocity, 4, 5, "extrapolation")
    assert np.array_equal(alone.to_host(), rate, equal_nan=True)


def test_units_mm_and_host_input():
    """Accumulations: ``/ accutime * 60.0`` on both sides, float64 host frames in and an ndarray out."""
    frames, velocity, nwp, meta = _whole_call_inputs()
    meta = dict(meta, transform=None, unit="mm", accutime=5, threshold=0.01, zerovalue=0.0)
    depth = np.where(frames[1] > -15, 10.0 ** (frames[1] / 10.0) / 12.0, 0.0).astype(np.float32)
    nwp_meta = dict(RATE_META, unit="mm", accutime=15)
    sch = dict(timesteps=4, timestep=5, start_blending=5, end_blending=20)
    got = lb().forecast(depth, meta, velocity, sch["timesteps"], sch["timestep"], "extrapolation", precip_nwp=nwp[0],
                        precip_nwp_metadata=nwp_meta, start_blending=5, end_blending=20)
    from pysteps_amd.nowcasts import get_method as nowcast_method

    nowcast = nowcast_method("extrapolation")(depth, velocity, 4)
    want = hb.blend(nowcast / float(5) * 60.0, nwp[0] / float(15) * 60.0, **sch)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and np.array_equal(got, want)


def test_db_inverse_float64_within_five_times_the_references_own_deviation(golden, bars):
    db = hb.db_field()
    assert hb.digest(db) == str(golden["db__sha256"])
    want = golden["db__rainrate"]
    got = lb().to_rainrate(dev(db), hb.DB_META).to_host()
    assert got.dtype == np.float64 and np.array_equal(np.isnan(got), np.isnan(want))
    threshold = 10.0 ** (hb.DB_META["threshold"] / 10.0)
    bar_ulp = 5.0 * bars["db_inverse_f64_own_deviation_ulp"]
    ok = np.isfinite(want)
    near = ok & (want > 0) & (np.abs(want - threshold) <= bar_ulp * np.spacing(threshold)) & (db != hb.DB_META["threshold"])
    assert np.count_nonzero(near) <= 1e-3 * want.size
    keep = ok & ~near
    assert np.array_equal(got[keep] == 0, want[keep] == 0)
    worst = np.max(np.abs(got[keep] - want[keep]) / np.spacing(np.maximum(want[keep], threshold)))
    print("float64 dB inverse: worst %.3f ulp against a bar of %.3f, %d pixels left out" % (worst, bar_ulp, np.count_nonzero(near)))
    assert worst <= bar_ulp


def test_short_nwp_raises_the_references_exception(golden):
    nowcast, nwp, kwargs = hb.make_case("single_37x53")
    exc = {"IndexError": IndexError}[str(golden["short_nwp_exception"])]
    with pytest.raises(exc):
        lb().blend(nowcast, nwp[:2], **kwargs)
    with pytest.raises(exc):
        lb().blend(dev(nowcast), dev(nwp[:2]), saliency=True, **kwargs)
    frames, velocity, nwp4, meta = _whole_call_inputs()
    with pytest.raises(exc):
        lb().forecast(frames, meta, velocity, 5, 5, "extrapolation", precip_nwp=nwp4[:, :3], precip_nwp_metadata=RATE_META,
                      start_blending=5, end_blending=20)


def test_declined_units_and_non_finite_maximum(ref_pysteps):
    """dBZ metadata and a salient lead time with an infinite maximum: the reference's result with a RuntimeWarning for
    host input, NotImplementedError for resident input."""
    import pysteps.nowcasts.interface as now_if
    from pysteps.blending.linear_blending import forecast as ref_forecast

    nowcast, nwp, kwargs = hb.make_case("single_37x53")
    frame = np.zeros(nowcast.shape[-2:])
    prepared = {"stack": nowcast}
    now_if._nowcast_methods["prepared_stack"] = lambda precip, velocity, timesteps, **kw: prepared["stack"].copy()
    try:
        args = (kwargs["timesteps"], kwargs["timestep"], "prepared_stack")
        kw = dict(precip_nwp=nwp, start_blending=kwargs["start_blending"], end_blending=kwargs["end_blending"])
        dbz = {"transform": None, "unit": "dBZ", "threshold": 5.0, "zerovalue": 0.0}
        for meta, nwp_meta, saliency in ((dbz, RATE_META, False), (RATE_META, dbz, False), (RATE_META, RATE_META, True)):
            if saliency:
                prepared["stack"] = nowcast.copy()
                prepared["stack"][1, 20, 20] = np.inf
            with warnings.catch_warnings(), np.errstate(all="ignore"):
                warnings.simplefilter("ignore")
                want = ref_forecast(frame, meta, None, *args, precip_nwp_metadata=nwp_meta, saliency=saliency, **kw)
            with pytest.warns(RuntimeWarning, match="running the reference's function"), np.errstate(all="ignore"):
                got = lb().forecast(frame, meta, None, *args, precip_nwp_metadata=nwp_meta, saliency=saliency, **kw)
            assert np.array_equal(got, want, equal_nan=True)
            with pytest.raises(NotImplementedError):
                lb().forecast(dev(frame), meta, None, *args, precip_nwp_metadata=nwp_meta, saliency=saliency, **kw)
    finally:
        del now_if._nowcast_methods["prepared_stack"]
