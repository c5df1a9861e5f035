"""The pointwise oracle of the extrapolator's resampling (helpers/semilag_pointwise.py), checked on the CPU against the
reference alone.

1. ``helpers.semilag_pointwise.resample`` IS the reference's resampling: at the displacement stored with every golden
   case of the unmodified reference it returns the golden's last plane to float64 round-off.
2. The skip rules skip next to nothing on the cases the device is held to (at the oracle's own displacement).
3. The ``C_k`` of tests/golden/semilag_pointwise_bars.json are reproducible and the bars derived from them stay below the
   pointwise equivalent of the 1e-4 contract.
4. The check has teeth: one interior pixel moved by twice its bar fails it, while the whole-plane relative L2 that
   tests/test_semilag_gpu.py holds fields to does not notice.
"""

import os

import numpy as np
import pytest

from conftest import GOLDEN, GoldenCases, rel_l2
from helpers import semilag_pointwise as pw
from helpers import semilag_pointwise_cases as pc

GOLDEN_FILES = ("semilag_reference.npz", "semilag_order3_modes.npz", "semilag_spline_orders.npz", "semilag_xy_coords.npz")


def _golden_cases():
    out = []
    for fname in GOLDEN_FILES:
        g = GoldenCases(os.path.join(GOLDEN, fname))
        for name in g.names:
            c = g.case(name)
            if "disp" in c and "out" in c and "precip" in c:
                out.append(pytest.param(name, c, id="%s-%s" % (fname.split(".")[0], name)))
    return out


_GOLDEN = _golden_cases()
# the goldens that skip more than ``skip_cap``: their motion fields are built from decimal constants, and the float32
# rounding of such a constant times the lead time puts whole rows of samples 1e-8 px off a .5 tie
_GOLDEN_SKIPS = {"sl_mode_gridwrap_o0": 20, "sl_mode_reflect_o0": 20}  # of 6912 pixels each; every other golden: skip_cap


def test_every_golden_file_contributes():
    ids = [p.id for p in _GOLDEN]
    for fname in GOLDEN_FILES:
        assert any(i.startswith(fname.split(".")[0]) for i in ids), fname
    assert len(ids) >= 40


@pytest.mark.parametrize("name,c", _GOLDEN)
def test_resample_is_the_reference(name, c):
    """The helper at the golden's displacement gives the golden's last plane: rtol 1e-12 (after the rounding to the
    field's dtype that SciPy's output array applies), identical NaN masks, next to nothing skipped."""
    kw = c["kw"]
    p = c["precip"]
    m, n = p.shape
    xy = kw.get("xy_coords", c.get("xy_coords"))
    order, mode = int(kw.get("interp_order", 1)), str(kw.get("map_coordinates_mode", "constant"))
    outval = kw.get("outval", np.nan)
    off = pw.grid_offsets(xy, m, n)
    want = c["out"][-1]
    got = pw.resample(p, c["disp"], order, mode, outval, off).astype(want.dtype)
    skip = pw.skip_mask(p, c["disp"], order, mode, outval, off)
    print("skipped", int(skip.sum()), "of", skip.size)
    assert skip.sum() <= _GOLDEN_SKIPS.get(name, pw.skip_cap(skip.size)), int(skip.sum())
    keep = ~skip
    assert np.array_equal(np.isnan(got[keep]), np.isnan(want[keep]))
    fin = keep & np.isfinite(want)
    assert fin.any() or np.isnan(want).all()
    np.testing.assert_allclose(got[fin], want[fin], rtol=1e-12, atol=0.0)
    # the magnitude bounds the sample of orders 0 / 1 (a convex combination of the taps)
    if order <= 1:
        mag = pw.magnitude(p, c["disp"], order, mode, outval, off)
        assert np.all(np.abs(want[fin].astype(np.float64)) <= mag[fin] * (1.0 + 1e-12))


_GROUPS = ([("low", o, mo) for o in (0, 1) for mo in pc.MODES] + [("spline", o, mo) for o in pc.SPLINE_ORDERS for mo in pc.MODES]
           + [("xy", None, None)])


def _group_cases(kind, order, mode):
    if kind == "xy":
        return pc.xy_cases()
    return pc.low_order_cases(order, mode) if kind == "low" else pc.spline_cases(order, mode)


@pytest.mark.parametrize("kind,order,mode", _GROUPS)
def test_skip_cap_holds_at_the_oracle_displacement(kind, order, mode):
    """Every device case (helpers/semilag_pointwise_cases.py) skips at most max(2, 1e-3 x pixels) when the oracle's own displacement is used, for each
    prefix of its lead times."""
    for case in _group_cases(kind, order, mode):
        kw = case["kw"]
        for k in range(1, pc.n_leads(case) + 1):
            disp = pc.oracle_displacement(case, k)
            skip = pw.skip_mask(case["precip"], disp, kw["interp_order"], kw["map_coordinates_mode"], kw["outval"],
                                pc.grid_off(case))
            assert skip.sum() <= pw.skip_cap(skip.size), (case["name"], k, int(skip.sum()))


def test_cases_cover_what_they_should():
    cases = list(pc.all_cases())
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    low = [c for c in cases if c["kw"]["interp_order"] <= 1 and "xy_coords" not in c["kw"]]
    assert {(c["kw"]["interp_order"], c["kw"]["map_coordinates_mode"], c["precip"].shape) for c in low} == {
        (o, mo, s) for o in (0, 1) for mo in pc.MODES for s in pc.LOW_SHAPES}
    for token in pc.FLOWS + pc.NAN_PLACEMENTS + ("K0", "K1", "K3", "-nan", "--15.0", "-min", "-frac", "-resumed"):
        assert any(token in c["name"] for c in low), token
    spl = [c for c in cases if c["kw"]["interp_order"] > 1 and "xy_coords" not in c["kw"]]
    assert {(c["kw"]["interp_order"], c["kw"]["map_coordinates_mode"], c["precip"].shape,
             bool(np.isnan(c["precip"]).any())) for c in spl} == {
        (o, mo, s, nan) for o in pc.SPLINE_ORDERS for mo in pc.MODES for s in pc.SPLINE_SHAPES for nan in (False, True)}
    assert sum("nancval" in c["name"] for c in spl) == len(pc.SPLINE_ORDERS)
    for c in cases:
        assert c["precip"].dtype == np.float32 and c["velocity"].dtype == np.float32 and np.isfinite(c["precip"]).any()


@pytest.mark.parametrize("order", pc.SPLINE_ORDERS)
def test_ck_measurement_is_reproducible(order):
    """Recomputing ``C_k`` gives the value in the JSON, to the four digits it stores; the bar is 4 x that and stays below
    the pointwise equivalent of the contract, 1e-4 x rms(field), of every case it applies to."""
    rec = pw.load_bars()["orders"][str(order)]
    ck, where, contract = pc.measure_ck(order)
    assert pc.stored(ck) == rec["C_k"], (ck, rec["C_k"], where)
    assert where == rec["worst_case"]
    assert rec["bar"] == pytest.approx(pw.BAR_FACTOR * rec["C_k"], rel=1e-12)
    assert pw.bar_ulps(order) == rec["bar"]
    assert pc.stored(contract) == rec["contract_ulps"]
    assert rec["bar"] < contract, (rec["bar"], contract)


def test_low_order_bars():
    assert pw.bar_ulps(0) == 0.0 and pw.bar_ulps(1) == 8.0


@pytest.mark.parametrize("order,mode", [(0, "constant"), (1, "constant"), (1, "reflect"), (3, "constant"), (5, "nearest")])
def test_the_check_has_teeth(order, mode):
    """One interior pixel of an oracle plane moved by twice its bar (order 0: by one float32 ulp): the pointwise check
    fails, the relative L2 under the 1e-4 contract and under the floor of test_semilag_gpu.py's regression bar (5e-7)
    still passes - the gap this file closes.  The untouched plane passes, so it is the pixel that is caught."""
    cases = pc.low_order_cases(order, mode) if order <= 1 else pc.spline_cases(order, mode)
    case = next(c for c in cases if c["precip"].shape in ((257, 131), (600, 523)))
    disp = pc.oracle_displacement(case, pc.n_leads(case))
    ref = pc.reference_at(case, disp)
    plane = ref.want.astype(np.float32)
    worst, _ = pw.pointwise_check(plane, ref)
    assert worst <= 1.0
    inner = np.isfinite(ref.want) & ~ref.skip & (ref.mag > 0)
    inner[:8] = inner[-8:] = False
    inner[:, :8] = inner[:, -8:] = False
    r, c = np.argwhere(inner)[inner.sum() // 2]
    faulty = plane.copy()
    if order == 0:
        faulty[r, c] = np.nextafter(faulty[r, c], np.float32(np.inf))
    else:
        # twice the bar, and at least two ulps of the value so that the float32 plane can hold the change
        faulty[r, c] += np.float32(max(2.0 * ref.bar[r, c], 4.0 * pw.EPS32 * abs(float(plane[r, c]))))
        assert abs(float(faulty[r, c]) - ref.want[r, c]) > ref.bar[r, c]
    with pytest.raises(AssertionError, match="pointwise"):
        pw.pointwise_check(faulty, ref)
    err = rel_l2(faulty, ref.want)
    assert err < 5e-7 < 1e-4, err  # test_semilag_gpu.py::_field_bar: min(max(5 x seen, 5e-7), 1e-4)
    assert np.array_equal(np.isnan(faulty), np.isnan(ref.want))
