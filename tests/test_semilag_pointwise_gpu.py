"""Every pixel of the single-field extrapolator's resampling (csrc/semilag.hip, semilag_device.h, spline.hip) against a
float64 oracle.

The advected fields of tests/test_semilag_gpu.py are held by a whole-plane relative L2, which does not see an error
confined to a few pixels: a window seam, a prefilter segment seam, the 12-sample padding of "nearest" / "grid-constant",
one folded tap of a boundary mode, the weight-0 x NaN rule at column n.  Here the last plane of a call is compared pixel by
pixel with the reference's resampling (helpers/semilag_pointwise.py, float64 SciPy) AT THE DISPLACEMENT THAT SAME CALL
RETURNED - an integer plus a float32 fraction, exact in a double - which takes trajectory drift out of the comparison.
The bars are a float32 rounding budget: equality for order 0, 8 u mag for order 1, 4 C_k u mag for orders 2 .. 5 with C_k
measured on the CPU against the reference only (tests/golden/semilag_pointwise_bars.json).

Per case: calls with k = 1 .. T lead times; the last plane of call k at call k's displacement; plane k - 1 of the T-step call
bit for bit equal to it; every prefix displacement within ``_disp_budget`` of the float64 oracle's.  Per case the routes
NumPy in, DeviceArray in, ``semilag_variant`` 7 and 12 and, where ``parallel.tiled_extrapolate`` takes the arguments, one
row band.  The cases are those of helpers/semilag_pointwise_cases.py (tests/test_semilag_pointwise_cpu.py shows that the
skip rules stay within their cap on each).  What was seen is appended to semilag_pointwise_seen.jsonl in the directory
named by PYSTEPS_HIP_SEEN_DIR, when that is set.

The bars were set before any device run and rest on the CPU measurement alone.  Where the device misses one, that is a
finding about the kernel or about the float32 restatement, to be explained next to the kernel in DESIGN.md with the failing
input kept as a named case - not a reason to widen a bar or a skip rule.
"""

import json
import os

import numpy as np
import pytest

from helpers import semilag_pointwise as pw
from helpers import semilag_pointwise_cases as pc

pytestmark = pytest.mark.gpu

ROUTES = ("numpy", "device", "variant7", "variant12", "band")


def _seen(rec):
    out_dir = os.environ.get("PYSTEPS_HIP_SEEN_DIR")
    if not out_dir:
        return
    try:
        os.makedirs(out_dir, exist_ok=True)
        rec = dict(rec, test=os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0])
        with open(os.path.join(out_dir, "semilag_pointwise_seen.jsonl"), "a") as fh:
            fh.write(json.dumps(rec) + "\n")
    except OSError:
        pass


@pytest.fixture(scope="module")
def extrapolate():
    from pysteps_amd.extrapolation import get_method

    return get_method("semilagrangian")


def _call(extrapolate, route, case, timesteps):
    """One call through a route -> (planes (k, m, n) float32, displacement (2, m, n) float64), on the host."""
    from pysteps_amd import _lib
    from pysteps_amd.device import DeviceArray

    kw = dict(case["kw"])
    p, v = case["precip"], case["velocity"]
    if route == "device":
        kw.pop("allow_nonfinite_values")  # the device-resident entry point scans nothing
        if "displacement_prev" in kw:
            kw["displacement_prev"] = DeviceArray.from_host(np.ascontiguousarray(kw["displacement_prev"], dtype=np.float64))
        out, disp = extrapolate(DeviceArray.from_host(p), DeviceArray.from_host(v), timesteps, return_displacement=True, **kw)
        return np.array(out.to_host()), np.array(disp.to_host())
    variant = {"variant7": 7, "variant12": 12}.get(route, 0)
    lib = _lib.lib()
    if variant:
        _lib.check(lib.psh_set_option(b"semilag_variant", variant))
    try:
        out, disp = extrapolate(p, v, timesteps, return_displacement=True, **kw)
    finally:
        _lib.check(lib.psh_set_option(b"semilag_variant", 0))
    return np.array(out), np.array(disp)


def _band_applies(case):
    kw = case["kw"]
    return (kw["map_coordinates_mode"] == "constant" and not isinstance(kw["outval"], str) and "xy_coords" not in kw
            and "displacement_prev" not in kw and case["precip"].shape[0] >= 3)


class _Refs:
    """The float64 references of one case, one per distinct displacement (the routes return the same bytes as a rule,
    so a case costs one resampling per lead time, not one per route)."""

    def __init__(self, case):
        self.case, self.cache = case, []

    def at(self, disp):
        for d, ref in self.cache:
            if np.array_equal(d, disp, equal_nan=True):
                return ref
        ref = pc.reference_at(self.case, disp)
        self.cache.append((disp.copy(), ref))
        return ref


def _check_case(extrapolate, case, stats):
    from pysteps_amd import parallel
    from pysteps_amd.device import DeviceArray

    T = pc.n_leads(case)
    m, n = case["precip"].shape
    refs = _Refs(case)
    wdisps = [pc.oracle_displacement(case, k) for k in range(1, T + 1)]
    bars = [pc.disp_bar(case, k) for k in range(1, T + 1)]
    worst, skipped, dworst = 0.0, 0, 0.0
    for route in ROUTES:
        if route == "band":
            if not _band_applies(case):
                continue
            # rows of the second of three bands, resampled at the displacement the resident call returned for them
            kw = case["kw"]
            rows, band = parallel.tiled_extrapolate(DeviceArray.from_host(case["precip"]), DeviceArray.from_host(case["velocity"]),
                                                    case["timesteps"], 1, 3, outval=kw["outval"], n_iter=kw["n_iter"],
                                                    interp_order=kw["interp_order"])
            band = np.array(band.to_host())
            full, gdisp = _call(extrapolate, "device", case, case["timesteps"])
            assert band.shape == (T, len(rows), n) and len(rows) > 0
            plane = np.full((m, n), np.nan, np.float32)
            ref = refs.at(gdisp)
            inside = np.zeros((m, n), bool)
            inside[rows.start: rows.stop] = True
            plane[inside] = band[-1].ravel()
            plane[~inside] = ref.want[~inside].astype(np.float32)  # only the band's rows are under test
            plane[~inside & np.isnan(ref.want)] = np.nan
            w, s = pw.pointwise_check(plane, ref)
            worst, skipped = max(worst, w), max(skipped, s)
            assert np.array_equal(band, full[:, rows.start: rows.stop], equal_nan=True), ("band", case["name"])
            continue
        full = None
        for k in range(T, 0, -1):
            out, gdisp = _call(extrapolate, route, case, pc.prefix(case, k))
            assert out.shape == (k, m, n) and out.dtype == np.float32 and gdisp.shape == (2, m, n)
            if k == T:
                full = out
            note = (case["name"], route, "k", k)
            # trajectories: each prefix displacement against the float64 oracle's
            wd = wdisps[k - 1]
            assert np.array_equal(np.isnan(gdisp), np.isnan(wd)), note + ("lost trajectories differ",)
            sane = np.isfinite(wd)
            if sane.any():
                derr = float(np.max(np.abs(gdisp[sane] - wd[sane])))
                dworst = max(dworst, derr / bars[k - 1])
                assert derr < bars[k - 1], note + ("trajectory", derr, bars[k - 1])
            # resampling: the last plane of call k at call k's own displacement
            ref = refs.at(gdisp)
            try:
                w, s = pw.pointwise_check(out[-1], ref)
                worst, skipped = max(worst, w), max(skipped, s)
                # plane k - 1 of the T-step call: the same check at the same displacement, and the same bytes
                w, s = pw.pointwise_check(full[k - 1], ref)
            except AssertionError as exc:
                raise AssertionError(note + exc.args) from None
            worst = max(worst, w)
            assert np.array_equal(full[k - 1], out[-1], equal_nan=True), note + ("plane k - 1 of the T-step call differs",)
    stats["worst"] = max(stats.get("worst", 0.0), worst)
    stats["skipped"] = max(stats.get("skipped", 0), skipped)
    stats["skip_share"] = max(stats.get("skip_share", 0.0), skipped / float(m * n))
    stats["disp"] = max(stats.get("disp", 0.0), dworst)
    _seen(dict(case=case["name"], order=case["kw"]["interp_order"], mode=case["kw"]["map_coordinates_mode"],
               err_in_bars=worst, skipped=skipped, pixels=m * n, disp_in_bars=dworst))


def _run(extrapolate, cases):
    stats = {}
    for case in cases:
        _check_case(extrapolate, case, stats)
    print("pointwise: worst %.3f of its bar, skipped <= %d (%.2e of a plane), displacement %.3f of its budget"
          % (stats["worst"], stats["skipped"], stats["skip_share"], stats["disp"]))


@pytest.mark.parametrize("mode", pc.MODES)
@pytest.mark.parametrize("order", [0, 1])
def test_low_orders_pointwise(extrapolate, order, mode):
    """Orders 0 (equality) and 1 (8 u mag over the 2 x 2 footprint) x the seven modes on 5 x 3 .. 257 x 131: the hard flows,
    NaN borders, NaNs in the last two rows / columns, a NaN hole in the motion field, n_iter 0 / 1 / 3, outval NaN / -15 /
    "min", fractional lead times and a resumed displacement (helpers/semilag_pointwise_cases.py::low_order_cases)."""
    _run(extrapolate, pc.low_order_cases(order, mode))


@pytest.mark.parametrize("mode", pc.MODES)
@pytest.mark.parametrize("order", pc.SPLINE_ORDERS)
def test_spline_orders_pointwise(extrapolate, order, mode):
    """Orders 2 .. 5 x the seven modes across the prefilter's 512-sample seams on each axis (530 x 70, 70 x 1030,
    600 x 523) and on a 40 x 56 control below every seam, with and without NaNs (zeroed samples across the seams), outval
    NaN and -15, "grid-constant" also with a NaN cval: 4 C_k u mag per pixel."""
    _run(extrapolate, pc.spline_cases(order, mode))


def test_custom_grids_pointwise(extrapolate):
    """A warped and a half-pixel staggered ``xy_coords`` at orders 0, 1 and 3: the coordinates are
    xy_coords + displacement formed in float64, as the reference forms them."""
    _run(extrapolate, pc.xy_cases())
