"""The transforms and unit conversions on resident fields (csrc/elementwise.hip psh_field_transform_dev, csrc/nqt.hip)
against the NumPy restatement of helpers/transforms.py.

Decisions on the input, counts, the square root and the square, the accumulation scalings, metadata and the inverse
interpolation are exact.  Values that go through a transcendental are held to tests/golden/transforms_bars.json: 5 x the
deviation the unmodified reference itself shows (float32: from the float64 value, in float32 spacings; float64: from
the exact value, in units of 2^-52; ndtri: in units of 2^-52 max(1, |value|)).  The inverse Box-Cox decision compares a
computed value: it is exact outside the bar of the threshold.
"""

import ctypes
import functools
import warnings

import numpy as np
import pytest

from helpers import elementwise as ew
from helpers import transforms as ht

pytestmark = pytest.mark.gpu

SMALL = ht.small_cases()
FAMILIES = [(tag, n, seed, dtype) for tag, n, seed, dtype in (
    ("n1", 1, 3001, np.float32), ("n1", 1, 4001, np.float64), ("n3", 3, 3003, np.float32), ("n3", 3, 4003, np.float64),
    ("stride", ht.GRID_STRIDE, 5000, np.float32), ("stride", ht.GRID_STRIDE, 6000, np.float64))]
FAMILY_SIZE = 2 * len(ht.LAMBDAS) + 2 * len(ht.ZR_LAWS)
GOLD = np.load(ht.REFERENCE_NPZ, allow_pickle=False)


def _dev(a):
    from pysteps_amd.device import DeviceArray

    return DeviceArray.from_host(np.ascontiguousarray(a))


def _host(d):
    return d.to_host(out=np.empty(d.shape, d.dtype))


def _quiet(fn, *args, **kwargs):
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*args, **kwargs)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_bits(a, b):
    """Bit for bit, NaN matching NaN."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    return np.array_equal(nan_a, nan_b) and np.array_equal(_bits(a)[~nan_a], _bits(b)[~nan_b])


def _run(case, field_dev):
    """The case's pass on a resident field, through the public functions."""
    from pysteps_amd import utils
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.utils import conversion

    if case.kind == "boxcox":
        out, _ = _quiet(utils.boxcox_transform, field_dev, {"transform": None}, Lambda=case.p0, threshold=case.threshold,
                        zerovalue=case.zerovalue)
    elif case.kind == "boxcox_inverse":
        out, _ = _quiet(utils.boxcox_transform, field_dev, {"transform": "BoxCox"}, Lambda=case.p0, threshold=case.threshold,
                        zerovalue=case.zerovalue, inverse=True)
    elif case.kind == "z_to_rate":
        out, _ = _quiet(utils.to_rainrate, field_dev, {"transform": None, "unit": "dBZ", "threshold": 1.0, "zerovalue": 0.0},
                        zr_a=case.p0, zr_b=case.p1)
    else:
        out = conversion._rate_to_z(field_dev, case.p0, case.p1)
    assert isinstance(out, DeviceArray) and out.dtype == case.dtype
    return _host(out)


@functools.lru_cache(maxsize=1)
def _family(index):
    tag, n, seed, dtype = FAMILIES[index]
    out = []
    ht._add_family(out, tag, n, seed, dtype)
    assert len(out) == FAMILY_SIZE
    return out


# ---- element-wise passes ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_elementwise_small(case):
    got = _run(case, _dev(case.R))
    dev = ht.hold(case, got, ht.bar(case.key))
    golden = GOLD[case.name + "__out"]
    assert np.array_equal(np.isnan(got), np.isnan(golden))  # NaN in gives NaN out, and what NumPy makes NaN is NaN
    print("%-40s worst deviation %.3f (bar %.2f)" % (case.name, dev, ht.bar(case.key)))


@pytest.mark.parametrize("member", range(FAMILY_SIZE))
@pytest.mark.parametrize("family", range(len(FAMILIES)), ids=["%s-%s" % (f[0], np.dtype(f[3]).name) for f in FAMILIES])
def test_elementwise_sizes(family, member):
    """n = 1 and n = 3 (tail only), and 2 100 003: vector body, tail and the grid stride over many blocks."""
    case = _family(family)[member]
    got = _run(case, _dev(case.R))
    dev = ht.hold(case, got, ht.bar(case.key))
    print("%-40s n=%-8d worst deviation %.3f (bar %.2f)" % (case.name, case.R.size, dev, ht.bar(case.key)))


def test_elementwise_plane_off_alignment_has_the_same_bits():
    """A plane view that does not start on a 16-byte boundary takes the one-element path: same bits as the aligned copy."""
    from pysteps_amd import utils

    planes = ht.stack()
    stack_dev = _dev(planes)
    view, copy = stack_dev.view(1), _dev(planes[1])
    assert view.ptr % 16 != 0 and copy.ptr % 16 == 0
    thr_t = ht.forward_threshold(0.1, 0.3)
    calls = [
        lambda f: utils.boxcox_transform(f, {"transform": None}, Lambda=0.3, threshold=0.1)[0],
        lambda f: utils.boxcox_transform(f, {"transform": None}, Lambda=0.0, threshold=0.1)[0],
        lambda f: utils.boxcox_transform(f, {"transform": "BoxCox"}, Lambda=0.3, threshold=thr_t, inverse=True)[0],
        lambda f: utils.sqrt_transform(f)[0],
        lambda f: utils.sqrt_transform(f, inverse=True)[0],
        lambda f: utils.to_rainrate(f, {"transform": None, "unit": "dBZ", "threshold": 1.0, "zerovalue": 0.0})[0],
        lambda f: utils.to_raindepth(f, {"transform": None, "unit": "mm/h", "threshold": 0.1, "zerovalue": 0.0, "accutime": 5})[0],
    ]
    for call in calls:
        a, b = _host(_quiet(call, view)), _host(_quiet(call, copy))
        assert a.shape == planes[1].shape and _same_bits(a, b)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_sqrt_and_square_are_exact(dtype):
    from pysteps_amd import utils

    R = np.concatenate([ht.specials(dtype), ht.field(ht.GRID_STRIDE, 81, dtype)])
    out, meta = utils.sqrt_transform(_dev(R))
    want, want_meta = ht.sqrt_transform(R)
    assert _same_bits(_host(out), want)
    assert meta["transform"] == "sqrt" and np.isnan(meta["zerovalue"]) and np.isnan(meta["threshold"])  # metadata=None
    given = {"transform": "sqrt", "zerovalue": 0.5, "threshold": 2.0}
    back, meta = utils.sqrt_transform(out, given, inverse=True)
    want_back, want_meta = ht.sqrt_transform(want, given, inverse=True)
    assert _same_bits(_host(back), want_back) and meta == want_meta == {"transform": None, "zerovalue": 0.25, "threshold": 4.0}
    for n in (1, 3):
        assert _same_bits(_host(utils.sqrt_transform(_dev(R[6:6 + n]))[0]), _quiet(np.sqrt, R[6:6 + n]))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_accumulation_scalings_are_exact(dtype):
    """R / float(accutime) * 60.0 and R / 60.0 * accutime: two correctly rounded operations in the field's dtype."""
    from pysteps_amd import utils

    R = np.concatenate([ht.specials(dtype), ht.field(ht.GRID_STRIDE, 82, dtype)])
    for accutime in (5, 7, 15.0):
        meta = {"transform": None, "unit": "mm", "threshold": 0.1, "zerovalue": 0.0, "accutime": accutime}
        rate, m1 = utils.to_rainrate(_dev(R), meta)
        want, want_m1 = ht.to_rainrate(R, meta)
        assert _same_bits(_host(rate), want) and m1 == want_m1 and m1["unit"] == "mm/h"
        depth, m2 = utils.to_raindepth(rate, m1)
        want2, want_m2 = ht.to_raindepth(want, want_m1)
        assert _same_bits(_host(depth), want2) and m2 == want_m2 and m2["unit"] == "mm"


# ---- counts ---------------------------------------------------------------------------------------------------------------


def _count_le(field_dev):
    """(counts, sorted values, number of values that are not NaN, min, max) from psh_nqt_count_le_dev."""
    from pysteps_amd import _lib
    from pysteps_amd.device import DeviceArray

    count = DeviceArray(field_dev.shape, np.uint32)
    ordered = DeviceArray((field_dev.size,), field_dev.dtype)
    n_valid, lo, hi = ctypes.c_size_t(), ctypes.c_double(), ctypes.c_double()
    _lib.check(_lib.lib().psh_nqt_count_le_dev(field_dev.ptr, int(field_dev.dtype == np.float32), field_dev.size, count.ptr,
                                               ordered.ptr, ctypes.byref(n_valid), ctypes.byref(lo), ctypes.byref(hi), None),
               "psh_nqt_count_le_dev")
    return _host(count), _host(ordered), n_valid.value, lo.value, hi.value


COUNT_CASES = ht.count_cases()


@pytest.mark.parametrize("name", sorted(COUNT_CASES))
def test_count_le(name):
    x = COUNT_CASES[name]
    count, ordered, n_valid, lo, hi = _count_le(_dev(x))
    flat = x.ravel()
    ok = ~np.isnan(flat)
    want = np.zeros(flat.shape, np.uint32)
    want[ok] = np.searchsorted(np.sort(flat[ok]), flat[ok], side="right")
    assert count.dtype == np.uint32 and np.array_equal(count.ravel(), want)
    assert n_valid == np.count_nonzero(ok)
    assert np.array_equal(ordered[:n_valid], np.sort(flat[ok])) and np.all(np.isnan(ordered[n_valid:]))
    assert lo == flat[ok].min() and hi == flat[ok].max()
    if name == "257x259-quantised":
        assert count.max() == n_valid and np.count_nonzero(flat == 0) > 35000  # one run of ties of about 40 000
    if name == "signed-zeros":
        zeros = count.ravel()[flat == 0]
        assert zeros.size > 1000 and np.all(zeros == zeros[0])  # -0.0 and +0.0 in one run


def test_count_le_does_not_depend_on_the_plane():
    x = COUNT_CASES["257x259-quantised"]
    stack_dev = _dev(np.stack([x, np.flipud(x), x]))
    first, second = _count_le(stack_dev.view(0)), _count_le(stack_dev.view(2))
    alone = _count_le(_dev(x))
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[0], alone[0])  # the counts
    assert _same_bits(first[1], second[1]) and _same_bits(first[1], alone[1])  # the sorted values
    assert first[2:] == second[2:] == alone[2:]


# ---- normal-quantile transform ------------------------------------------------------------------------------------------


def _nq_field():
    return ht.rain_field((257, 259), 9, np.float32, nans=11)


@pytest.mark.parametrize("a", [0.0, 0.375])
def test_nq_forward(a):
    from pysteps_amd import utils
    from pysteps_amd.device import DeviceArray

    x = _nq_field()
    out, meta = utils.NQ_transform(_dev(x), a=a)
    assert isinstance(out, DeviceArray) and out.dtype == np.float64
    got = _host(out)
    want, want_meta = ht.NQ_transform(x, a=a)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got == 0, want == 0) and np.all(got[x == 0] == 0)
    dev = ht.within_ndtri_bar(got, want)
    print("NQ forward a=%s: worst deviation from SciPy's ndtri %.3f (bar %.2f)" % (a, dev, ht.bar("ndtri")))
    assert dev <= ht.bar("ndtri")
    assert type(meta["threshold"]) is type(want_meta["threshold"]) is np.float64
    assert abs(meta["threshold"] - want_meta["threshold"]) <= ht.bar("ndtri") * ht.EPS * max(1.0, abs(want_meta["threshold"]))
    assert meta["transform"] == "NQT" and meta["zerovalue"] == 0 and type(meta["zerovalue"]) is int
    # float32 on request: the float64 result rounded once
    narrow, meta32 = utils.NQ_transform(_dev(x), a=a, dtype=np.float32)
    assert narrow.dtype == np.float32 and _same_bits(_host(narrow), got.astype(np.float32))
    assert type(meta32["threshold"]) is np.float64 and meta32["threshold"] == np.float64(got.astype(np.float32)[got > 0].min())
    # the same bits in every run
    again, meta_again = utils.NQ_transform(_dev(x), a=a)
    assert _same_bits(_host(again), got) and meta_again["threshold"] == meta["threshold"]
    # a given zerovalue that no pixel has: no pixel is set to 0, the count rule alone
    plain, _ = utils.NQ_transform(_dev(x), {"transform": None, "zerovalue": -1.0}, a=a)
    want_plain, _ = ht.NQ_transform(x, {"transform": None, "zerovalue": -1.0}, a=a)
    assert ht.within_ndtri_bar(_host(plain), want_plain) <= ht.bar("ndtri")


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_nq_inverse(dtype):
    """With the device's own tables downloaded, interp1d's rule in NumPy gives the same bits."""
    from pysteps_amd import utils

    x = _nq_field()
    fwd_dev, meta = utils.NQ_transform(_dev(x), a=0.375)
    moved = ht.shifted(_host(fwd_dev))
    moved.flat[5], moved.flat[6], moved.flat[7] = -9.0, 9.0, 0.123  # below the table, above it, between two knots
    moved = moved.astype(dtype)
    f = meta["inqt"]
    xs = _host(f.table())
    ys = _host(f.sorted_dev)[:f.n].astype(np.float64)
    assert np.all(np.diff(xs) > 0) and xs.size == f.n == np.count_nonzero(~np.isnan(x))
    back_dev, meta_back = utils.NQ_transform(_dev(moved), meta, inverse=True)
    back = _host(back_dev)
    ok = ~np.isnan(moved)
    assert back.dtype == np.float64 and np.array_equal(np.isnan(back), ~ok)
    want = ht.interp_linear(xs, ys, moved[ok].astype(np.float64))
    assert np.array_equal(back[ok], want)
    assert back.flat[5] == ys[0] and back.flat[6] == ys[-1]
    assert "inqt" in meta and "inqt" not in meta_back and meta_back["transform"] is None
    assert type(meta_back["zerovalue"]) is np.float64 and meta_back["zerovalue"] == want.min()
    assert type(meta_back["threshold"]) is np.float64 and meta_back["threshold"] == want[want > want.min()].min()
    # the object is also callable on a resident and on a NumPy array
    assert np.array_equal(_host(f(_dev(moved)))[ok], want)
    from scipy.interpolate import interp1d
    from scipy.special import ndtri

    reference_table = interp1d(ndtri(ht.plotting_positions(np.arange(f.n) + 1, f.n, 0.375)), ys, bounds_error=False,
                               fill_value=(ys[0], ys[-1]))
    assert np.array_equal(f(moved[ok].astype(np.float64)), reference_table(moved[ok].astype(np.float64)))


def test_nq_inverse_takes_a_host_interp1d():
    """A resident field with the metadata of a host forward transform: the interp1d's tables are uploaded."""
    from pysteps_amd import utils
    from pysteps_amd.device import DeviceArray

    x = ht.rain_field((48, 64), 21, np.float32, nans=5)
    fwd, meta = utils.NQ_transform(x, a=0.375)
    f = meta["inqt"]
    moved = ht.shifted(fwd)
    moved.flat[7], moved.flat[11] = -9.0, 9.0
    back_dev, meta_back = utils.NQ_transform(_dev(moved), meta, inverse=True)
    want, meta_want = utils.NQ_transform(moved, meta, inverse=True)
    assert isinstance(back_dev, DeviceArray) and "inqt" in meta and "inqt" not in meta_back
    assert _same_bits(_host(back_dev), want) and _same_metadata(meta_back, meta_want)
    assert np.array_equal(want[~np.isnan(moved)], ht.interp_linear(f.x, f.y, moved[~np.isnan(moved)]))


@pytest.mark.parametrize("a", [0.0, 0.375])
def test_nq_round_trip_against_the_reference(a):
    """Forward, a small shift, inverse: within the bar of the golden round trip, zeros-do-not-return quirk included."""
    from pysteps_amd import utils

    name = "nq-48x64-f32"
    x = ht.rain_field((48, 64), 21, np.float32, nans=5)
    tag = "%s__a%s" % (name, a)
    fwd_dev, meta = utils.NQ_transform(_dev(x), a=a)
    fwd = _host(fwd_dev)
    golden = GOLD[tag + "__forward"]
    assert np.array_equal(np.isnan(fwd), np.isnan(golden)) and np.array_equal(fwd == 0, golden == 0)
    assert ht.within_ndtri_bar(fwd, golden) <= ht.bar("ndtri")
    moved = ht.shifted(fwd)
    moved.flat[7], moved.flat[11] = -9.0, 9.0
    back_dev, meta_back = utils.NQ_transform(_dev(moved), meta, inverse=True)
    back, golden_back = _host(back_dev), GOLD[tag + "__inverse"]
    assert np.array_equal(np.isnan(back), np.isnan(golden_back))
    dev = ht.within_ndtri_bar(back, golden_back)
    print("NQ round trip a=%s: worst deviation from the reference %.3f (bar %.2f)" % (a, dev, ht.bar("ndtri")))
    assert dev <= ht.bar("ndtri")
    table_at_zero = ht.interp_linear(_host(meta["inqt"].table()), _host(meta["inqt"].sorted_dev)[:meta["inqt"].n], np.zeros(1))[0]
    zero_pixels = (moved == 0)
    assert zero_pixels.any() and np.all(back[zero_pixels] == table_at_zero)


# ---- conversions --------------------------------------------------------------------------------------------------------


def _same_metadata(a, b):
    return a.keys() == b.keys() and all(type(a[k]) is type(b[k]) and (a[k] == b[k] or (a[k] != a[k] and b[k] != b[k])) for k in a)


def test_conversion_chain_stays_resident():
    """dBZ composite -> to_rainrate -> dB_transform -> its inverse -> to_reflectivity, every output a DeviceArray.  Each
    function is compared with the helper's on the device's previous result.  A function that chains two passes (the dB
    inverse and the Z-R law, the Z-R law and the dB transform) is held pass by pass, the second from the device's own
    intermediate: the rounding of an intermediate near Z = 1 moves 10 log10 Z by many of its spacings in any
    implementation, so a bar for the pair would measure the input, not the arithmetic."""
    from pysteps_amd import utils
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.utils import conversion

    dbz = (10.0 * np.log10(ht.reflectivities(1031, 31, np.float64))).astype(np.float32)
    dbz[::7] = -15.0
    meta = {"transform": "dB", "unit": "dBZ", "threshold": -10.0, "zerovalue": -15.0, "accutime": 5}

    def check(k, out_dev, m_got, want, m_want, bar):
        assert isinstance(out_dev, DeviceArray) and out_dev.dtype == np.float32
        assert _same_metadata(m_got, m_want), (k, m_got, m_want)
        got = _host(out_dev)  # downloaded only to compare
        zv = np.float32(m_want["zerovalue"])
        assert np.array_equal(got == zv, want == zv), k
        dev, wrong = ew.deviation(got, want.astype(np.float64), want != zv)
        print("conversion chain step %s: worst deviation %.3f float32 spacings (bar %.2f)" % (k, dev, bar))
        assert wrong == 0 and dev <= bar
        return got

    # to_rainrate = the dB inverse, then the Z-R law
    lin_dev, m_lin = utils.dB_transform(_dev(dbz), meta, inverse=True)
    lin = check("0a", lin_dev, m_lin, *_quiet(ht.dB_transform, dbz, meta, inverse=True), ew.bar("inverse"))
    rate_dev, m_rate = utils.to_rainrate(_dev(dbz), meta)
    want, m_want = _quiet(ht.to_rainrate, lin, m_lin)
    rate = check("0b", rate_dev, m_rate, want, m_want, ht.bar("f32/z_to_rate"))
    # the dB transform and back
    db_dev, m_db = utils.dB_transform(rate_dev, m_rate)
    db = check("1", db_dev, m_db, *_quiet(ht.dB_transform, rate, m_rate), ew.bar("forward"))
    back_dev, m_back = utils.dB_transform(db_dev, m_db, inverse=True)
    back = check("2", back_dev, m_back, *_quiet(ht.dB_transform, db, m_db, inverse=True), ew.bar("inverse"))
    # to_reflectivity = the Z-R law, then the dB transform
    z_dev = conversion._rate_to_z(back_dev, 200.0, 1.6)
    z = _host(z_dev)
    dev, wrong = ew.deviation(z, ht.evaluate("rate_to_z", back, 200.0, 1.6, wide=np.float64))
    assert wrong == 0 and dev <= ht.bar("f32/rate_to_z")
    m_z = dict(m_back, threshold=200.0 * m_back["threshold"] ** 1.6, zerovalue=200.0 * m_back["zerovalue"] ** 1.6, zr_a=200.0, zr_b=1.6)
    want, m_want = _quiet(ht.dB_transform, z, m_z)
    m_want["unit"] = "dBZ"
    refl_dev, m_refl = utils.to_reflectivity(back_dev, m_back)
    check("3", refl_dev, m_refl, want, m_want, ew.bar("forward"))
    assert m_refl["unit"] == "dBZ" and m_refl["transform"] == "dB" and m_refl["zr_a"] == 200.0 and m_refl["zr_b"] == 1.6
    want_all, m_all = _quiet(ht.to_reflectivity, back, m_back)
    assert _same_metadata(m_refl, m_all)


def test_zr_law_other_than_marshall_palmer_is_recorded():
    from pysteps_amd import utils

    Z = ht.reflectivities(4099, 5, np.float32)
    meta = {"transform": None, "unit": "dBZ", "threshold": 1.0, "zerovalue": 0.0}
    out, m = utils.to_rainrate(_dev(Z), meta, zr_a=316.0, zr_b=1.5)
    want, m_want = ht.to_rainrate(Z, meta, zr_a=316.0, zr_b=1.5)
    assert _same_metadata(m, m_want) and m["zr_a"] == 316.0 and m["zr_b"] == 1.5 and m["unit"] == "mm/h"
    dev, wrong = ew.deviation(_host(out), ht.evaluate("z_to_rate", Z, 316.0, 1.5, wide=np.float64))
    assert wrong == 0 and dev <= ht.bar("f32/z_to_rate")


# ---- declines -----------------------------------------------------------------------------------------------------------


def test_declines():
    from pysteps_amd import _reference, utils

    x = ht.rain_field((16, 16), 3, np.float32)
    x[3, 3] = np.inf
    with pytest.raises(NotImplementedError, match="infinite values"):
        utils.NQ_transform(_dev(x))
    with pytest.raises(NotImplementedError, match="dtype int32"):
        utils.NQ_transform(_dev(np.arange(12, dtype=np.int32).reshape(3, 4)))
    with pytest.raises(NotImplementedError, match="dtype int32"):
        utils.boxcox_transform(_dev(np.arange(12, dtype=np.int32)), {"transform": None})
    with pytest.raises(NotImplementedError, match="float64 parameter with a float32 field"):
        utils.boxcox_transform(_dev(x), {"transform": None}, Lambda=np.float64(0.3))  # NumPy would widen the result
    if _reference.lookup("utils.transformation", "NQ_transform", utils.NQ_transform) is not None:
        with pytest.warns(RuntimeWarning, match="infinite values"):
            utils.NQ_transform(x)
    else:
        with pytest.raises(NotImplementedError, match="infinite values"):
            utils.NQ_transform(x)
