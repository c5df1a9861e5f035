"""The three outlier kernels of csrc/sparse_qc.hip against the exact yardstick of tests/helpers/outliers.py.

``launch_outliers`` picks ``outliers_local_sorted<16>`` up to 1024 vectors, ``outliers_local_sorted<32>`` up to 2048
and the rescanning ``outliers_local`` up to 8192; every parametrised id starts with the kernel it selects.  Each case
goes through the C entry ``psh_outliers_local_host`` (ctypes) and through ``detect_outliers_device``; the flags must
EQUAL the yardstick's - no flip allowance, the integer lattices with duplicate positions included - because every
case is a margin of 1e-6 (relative, in the Mahalanobis distance) away from the threshold, 1000 times the error of the
float64 one-pass formula (tests/test_outliers_cpu.py asserts both, tests/golden/outliers_margins.json records them).

Above 2100 vectors the yardstick is evaluated on 512 sampled rows plus rows 0, 63, 64 and n - 1; the device computes
every row.
"""

import warnings

import numpy as np
import pytest

from helpers import outliers as ho

pytestmark = pytest.mark.gpu


def c_entry(xy, uv, k, thr):
    """(rc, flags): psh_outliers_local_host exactly as pysteps_amd/utils/cleansing.py calls it."""
    from pysteps_amd import _lib

    xy = np.ascontiguousarray(xy, np.float64)
    uv = np.ascontiguousarray(uv, np.float64)
    n = xy.shape[0]
    flags = np.full(max(n, 1), 0xAA, np.uint8)  # a row the kernel forgets stays visible
    rc = _lib.lib().psh_outliers_local_host(xy.ctypes.data, uv.ctypes.data, n, int(k), float(thr), flags.ctypes.data)
    return rc, flags[:n]


def _mismatch(case, exp, got):
    bad = np.flatnonzero(got[exp.rows].astype(bool) != exp.flags)
    text = "; ".join("row %d: device %d, yardstick %d (md %.6g, singular %s)" % (
        exp.rows[b], got[exp.rows[b]], exp.flags[b], float(exp.md[b]), exp.singular[b]) for b in bad[:5])
    return len(bad), text


@pytest.mark.parametrize("name", ho.NAMES, ids=ho.IDS)
def test_flags_equal_the_yardstick(name):
    from pysteps_amd.utils import detect_outliers_device

    case, exp = ho.case(name), ho.expected(name)
    rc, got = c_entry(case.xy, case.uv, case.k, case.thr)
    assert rc == 0
    assert np.isin(got, (0, 1)).all(), "rows never written: %s" % np.flatnonzero(~np.isin(got, (0, 1)))[:5]
    bad, text = _mismatch(case, exp, got)
    print("%s: %d vectors, k=%d, %d of %d checked rows differ, %d flagged on the device" % (
        case.id, case.n, case.k, bad, len(exp.rows), int(got.sum())))
    assert bad == 0, text
    if case.kind == "collinear":
        assert not got.any(), "singular covariance flagged at rows %s" % np.flatnonzero(got)[:5]
    rc2, again = c_entry(case.xy, case.uv, case.k, case.thr)
    assert rc2 == 0 and again.tobytes() == got.tobytes()
    wrapped = detect_outliers_device(case.uv, case.thr, case.xy, case.k)
    assert wrapped.dtype == bool and wrapped.shape == (case.n,)
    assert wrapped.tobytes() == got.astype(bool).tobytes()


def test_large_coordinates_give_the_unshifted_flags():
    """Positions shifted by (2.6e5, 9.6e5): the differences are taken in float64, so nothing may change."""
    shifted, base = ho.case("large-n1025-k30"), ho.large_base()
    assert np.array_equal(shifted.xy - ho.LARGE_SHIFT, base.xy)
    rc_s, got_s = c_entry(shifted.xy, shifted.uv, 30, ho.THR)
    rc_b, got_b = c_entry(base.xy, base.uv, 30, ho.THR)
    assert rc_s == 0 and rc_b == 0
    assert got_s.tobytes() == got_b.tobytes()
    assert np.array_equal(got_b.astype(bool), ho.Expected(base).flags)


def test_near_ties_follow_the_float32_key():
    """Where two float64 distances round to one float32 the lower index wins, though it is the farther vector."""
    name = "neartie-n600-k8"
    case, exp = ho.case(name), ho.expected(name)
    rows = ho.near_tie_rows(case)
    assert len(rows) >= ho.NEAR_TIE_MIN
    rc, got = c_entry(case.xy, case.uv, case.k, case.thr)
    assert rc == 0
    by64 = ho.Expected(case, selector=ho.knn_by_float64)
    print("near ties: %d rows, float64-key flags differ from float32-key flags at %d rows" % (
        len(rows), int(np.count_nonzero(by64.flags != exp.flags))))
    assert np.array_equal(got.astype(bool), exp.flags)


def test_more_vectors_than_the_device_holds():
    from pysteps_amd import _lib
    from pysteps_amd.utils import detect_outliers, detect_outliers_device

    n = ho.MAX_N + 1
    rng = np.random.default_rng(8193)
    xy, uv = rng.uniform(0, 4096, (n, 2)), rng.normal(0, 1, (n, 2)) + [3, -2]
    uv[rng.choice(n, n // 30, replace=False)] += 7.0
    rc, _ = c_entry(xy, uv, 30, ho.THR)
    assert rc == _lib.PSH_EUNSUPPORTED
    assert np.array_equal(detect_outliers_device(uv, ho.THR, xy, 30), detect_outliers(uv, ho.THR, xy, 30))


def test_argument_limits():
    from pysteps_amd import _lib
    from pysteps_amd.utils import detect_outliers_device

    case = ho.case("cont-n31-k30")
    assert c_entry(case.xy, case.uv, 0, ho.THR)[0] == _lib.PSH_EINVAL
    assert c_entry(case.xy, case.uv, -3, ho.THR)[0] == _lib.PSH_EINVAL
    with pytest.raises(ValueError):
        detect_outliers_device(case.uv, ho.THR, case.xy, 0)
    # no vector: nothing is touched; one vector: not an outlier
    rc, none = c_entry(np.zeros((0, 2)), np.zeros((0, 2)), 30, ho.THR)
    assert rc == 0 and none.size == 0
    rc, one = c_entry(np.array([[5.0, 7.0]]), np.array([[3.0, -2.0]]), 30, ho.THR)
    assert rc == 0 and one.tolist() == [0]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert detect_outliers_device(np.zeros((0, 2)), ho.THR, np.zeros((0, 2)), 30).shape == (0,)
        assert detect_outliers_device(np.array([[3.0, -2.0]]), ho.THR, np.array([[5.0, 7.0]]), 30).tolist() == [False]
