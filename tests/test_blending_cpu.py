"""Linear and salient blending without a GPU: the helper's NumPy restatement against the goldens of the unmodified
reference (bit for bit), the host side of ``pysteps_amd.blending`` - weight schedule, member index map, method names,
registration - and the share of dB pixels near the threshold."""

import json
import os
from functools import partial

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import blending as hb


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "blending_reference.npz"))


@pytest.fixture(scope="module")
def bars():
    with open(os.path.join(GOLDEN, "blending_bars.json")) as f:
        return json.load(f)


def test_golden_records_numpy_and_cases(golden, bars):
    assert json.loads(str(golden["versions"]))["numpy"] == bars["numpy"] == "2.2.6"
    assert sorted(str(c) for c in golden["cases"]) == sorted(hb.CASES)
    assert str(golden["short_nwp_exception"]) == "IndexError"


@pytest.mark.parametrize("name", sorted(hb.CASES))
def test_restatement_equals_reference_bit_for_bit(golden, name):
    nowcast, nwp, kwargs = hb.make_case(name)
    assert hb.digest(nowcast, nwp) == str(golden[name + "__sha256"])
    assert json.loads(str(golden[name + "__args"])) == kwargs
    before = nowcast.copy(), nwp.copy()
    for saliency in (False, True):
        want = golden[name + ("__salient" if saliency else "__linear")]
        got = hb.blend(nowcast, nwp, saliency=saliency, **kwargs)
        assert got.shape == want.shape and got.dtype == want.dtype == nwp.dtype
        assert not np.isnan(want).any() and np.array_equal(got, want)
    assert np.array_equal(nowcast, before[0], equal_nan=True) and np.array_equal(nwp, before[1], equal_nan=True)


def test_salient_cases_differ_from_linear(golden):
    """The goldens tell the two methods apart, and joint ranking from ranking per member."""
    assert not np.array_equal(golden["plain_64x96__linear"], golden["plain_64x96__salient"])
    nowcast, nwp, kwargs = hb.make_case("ens3_40x50")
    per_member = np.stack([hb.blend(nowcast[k], nwp[k], saliency=True, **kwargs) for k in range(3)])
    assert not np.array_equal(per_member, golden["ens3_40x50__salient"])


def test_restatement_raises_on_a_short_nwp_stack(golden):
    nowcast, nwp, kwargs = hb.make_case("single_37x53")
    with pytest.raises(IndexError):
        hb.blend(nowcast, nwp[:2], **kwargs)


@pytest.mark.parametrize("args", [
    (24, 10, 120, 240),     # integer steps: t hits start (weight 0) and end (weight 1) exactly
    (5, 5, 5, 20),
    (8, 2.5, 5, 15),        # float steps that hit both ends
    (12, 0.1, 0.3, 0.9),    # float steps whose products are not exact
    (6, 7.5, 10, 33),
    (4, 5, 30, 60),         # all before the window
    (4, 30, 5, 20),         # all after it
])
def test_weight_schedule_is_the_references(args):
    from pysteps_amd.blending.linear_blending import weight_schedule

    timesteps, timestep, start, end = args
    want = []
    for i in range(timesteps):  # linear_blending.py:215-239
        t = (i + 1) * timestep
        w = (t - start) / (end - start)
        want.append(0.0 if w <= 0.0 else (1.0 if w >= 1.0 else w))
    got = weight_schedule(timesteps, timestep, start, end)
    assert got == want == hb.weights(timesteps, timestep, start, end)
    assert all(type(w) is float for w in got)
    if args[:2] == (24, 10):
        assert got[11] == 0.0 and got[12] > 0.0 and got[22] < 1.0 and got[23] == 1.0


@pytest.mark.parametrize("kn,kw", hb.PAIRINGS)
def test_member_map_equals_np_repeat(kn, kw):
    from pysteps_amd.blending.linear_blending import member_maps

    map_n, map_w = member_maps(kn, kw)
    want_n, want_w = hb.repeat_maps(kn, kw)
    assert np.array_equal(map_n, want_n) and np.array_equal(map_w, want_w)
    assert len(map_n) == len(map_w) == max(kn, kw)


def test_method_names():
    from pysteps_amd.blending import get_method
    from pysteps_amd.blending.linear_blending import forecast

    for name in ("linear_blending", "linear_blending_hip", "Linear_Blending_HIP"):
        assert get_method(name) is forecast
    for name in ("salient_blending", "salient_blending_hip"):
        fn = get_method(name)
        assert isinstance(fn, partial) and fn.func is forecast and fn.keywords == {"saliency": True}
    with pytest.raises(ValueError):
        get_method("steps")


def test_forecast_has_the_references_signature():
    import inspect

    from pysteps_amd.blending.linear_blending import blend, forecast

    params = inspect.signature(forecast).parameters
    assert list(params) == ["precip", "precip_metadata", "velocity", "timesteps", "timestep", "nowcast_method", "precip_nwp",
                            "precip_nwp_metadata", "start_blending", "end_blending", "fill_nwp", "saliency", "nowcast_kwargs"]
    defaults = {k: p.default for k, p in params.items() if p.default is not inspect.Parameter.empty}
    assert defaults == dict(precip_nwp=None, precip_nwp_metadata=None, start_blending=120, end_blending=240, fill_nwp=True,
                            saliency=False, nowcast_kwargs=None)
    assert list(inspect.signature(blend).parameters) == ["precip_nowcast", "precip_nwp", "timesteps", "timestep",
                                                         "start_blending", "end_blending", "fill_nwp", "saliency"]


def test_register_blending_against_a_fake_table(monkeypatch):
    import sys
    import types

    from pysteps_amd import register
    from pysteps_amd.blending.linear_blending import forecast

    stock = object()
    fake_if = types.ModuleType("pysteps.blending.interface")
    fake_if._blending_methods = {"linear_blending": stock, "salient_blending": stock}
    fake_blending = types.ModuleType("pysteps.blending")
    fake_blending.interface = fake_if
    fake_pysteps = types.ModuleType("pysteps")
    fake_pysteps.blending = fake_blending
    for name, mod in (("pysteps", fake_pysteps), ("pysteps.blending", fake_blending), ("pysteps.blending.interface", fake_if)):
        monkeypatch.setitem(sys.modules, name, mod)
    added = register.register_blending()
    assert added == ["blending:linear_blending_hip", "blending:salient_blending_hip"]
    table = fake_if._blending_methods
    assert table["linear_blending_hip"] is forecast
    assert table["salient_blending_hip"].func is forecast and table["salient_blending_hip"].keywords == {"saliency": True}
    assert table["linear_blending"] is stock and table["salient_blending"] is stock


def test_reference_alone_stays_inside_the_threshold_cap(golden, bars):
    """The dB test of the GPU file may leave out pixels whose reference value lies within the bar of the linear
    threshold, up to a share of 1e-3: on the 0.25 dB grid the reference's own values leave out none."""
    db = hb.db_field()
    assert hb.digest(db) == str(golden["db__sha256"])
    assert np.array_equal(np.round(db[np.isfinite(db)] * 4.0), db[np.isfinite(db)] * 4.0)
    rate = golden["db__rainrate"]
    threshold = 10.0 ** (hb.DB_META["threshold"] / 10.0)
    bar = 5.0 * bars["db_inverse_f64_own_deviation_ulp"] * np.spacing(threshold)
    near = np.isfinite(rate) & (np.abs(rate - threshold) <= bar) & (db != hb.DB_META["threshold"])
    assert np.count_nonzero(near) <= 1e-3 * rate.size
    assert 0.0 < bars["db_inverse_f64_own_deviation_ulp"] < 2.0
    assert np.count_nonzero(db == hb.DB_META["threshold"]) > 0 and np.all(rate[db == hb.DB_META["threshold"]] > 0)
