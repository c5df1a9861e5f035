"""The resident element-wise passes (csrc/elementwise.hip) against the NumPy restatement of helpers/elementwise.py,
element by element.

Decisions that compare an input (the forward zero mask, every reduction, the conversions, axpy) are exact.  The
transcendental values are held to 5 x the deviation the unmodified reference itself shows from the float64 value
(tests/golden/elementwise_bars.json, measured by tests/test_elementwise_cpu.py), in spacings of the float32 result.
The inverse decision compares a computed value: it is exact wherever the float64 value is further than that bar from
the threshold, and nearer elements must still be either ``zerovalue`` or within the bar of their value.

NaN results are compared as NaN, not by payload: which NaN an operation returns is not part of NumPy's contract either.
"""

import ctypes
import functools
import warnings

import numpy as np
import pytest

from helpers import elementwise as ew

pytestmark = pytest.mark.gpu

CASES = ew.cases()
FORWARD = [c for c in CASES if not c.inverse]
INVERSE = [c for c in CASES if c.inverse]


def _lib():
    from pysteps_amd import _lib as lib_mod

    return lib_mod


def _dev(a):
    from pysteps_amd.device import DeviceArray

    return DeviceArray.from_host(np.ascontiguousarray(a))


def _host(d):
    return d.to_host(out=np.empty(d.shape, d.dtype))


def _quiet(fn, *args, **kwargs):
    # forming 10 log10 of a zero or negative threshold warns on the host, as in the reference
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*args, **kwargs)


def _transform(field_dev, case):
    from pysteps_amd.utils import dB_transform

    out, meta = _quiet(dB_transform, field_dev, case.metadata(), threshold=case.threshold, zerovalue=case.zerovalue,
                       inverse=case.inverse)
    return _host(out), meta


@functools.lru_cache(maxsize=None)
def _result(index):
    """(float32 result, metadata) of case ``index`` on the device; computed once, read-only."""
    got, meta = _transform(_dev(CASES[index].R), CASES[index])
    got.setflags(write=False)
    return got, meta


def _got(case):
    return _result(CASES.index(case))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same_values(a, b):
    """Bit for bit, NaN matching NaN."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    return np.array_equal(nan_a, nan_b) and np.array_equal(_bits(a)[~nan_a], _bits(b)[~nan_b])


def _same_number(a, b):
    return a == b or (a != a and b != b)


def _same_metadata(a, b):
    return a.keys() == b.keys() and all(type(a[k]) is type(b[k]) and _same_number(a[k], b[k]) for k in a)


# ---- dB forward -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", FORWARD, ids=lambda c: c.name)
def test_db_forward(case):
    """The elements that received ``zerovalue`` are the restatement's, all of them; every other element is within the
    forward bar of the float64 value, NaN and the infinities exactly."""
    got, _ = _got(case)
    exp = ew.expectation(case)
    zeroed = got == np.float32(case.zerovalue)
    assert np.array_equal(zeroed, exp.zeros), np.flatnonzero(zeroed != exp.zeros)[:8]
    dev, wrong = ew.deviation(got, exp.value, ~exp.zeros)
    print("forward %-34s n=%-8d worst deviation %.3f spacings (bar %.2f)" % (case.name, case.R.size, dev, ew.bar("forward")))
    assert wrong == 0
    assert dev <= ew.bar("forward"), dev


def test_db_forward_special_values():
    sp = ew.rate_specials()
    zero_thr = next(c for c in FORWARD if c.name == "fwd-specials-thr0-float")
    got, _ = _got(zero_thr)
    assert np.all(np.isneginf(got[sp == 0.0])) and np.count_nonzero(sp == 0.0) == 2  # +0.0 and -0.0: log10(0) is kept
    assert np.all(np.isnan(got[np.isnan(sp)])) and np.all(np.isposinf(got[np.isposinf(sp)]))
    assert np.all(got[sp < 0] == np.float32(zero_thr.zerovalue))
    # the smallest normal and a subnormal are not flushed
    assert abs(float(got[sp == np.float32(ew.SUBNORMAL)][0]) + 400.0) < 1e-3
    assert abs(float(got[sp == np.float32(ew.FLT_MIN)][0]) - 10.0 * np.log10(ew.FLT_MIN)) < 1e-3
    negative_thr = next(c for c in FORWARD if c.name == "fwd-specials-thr-1-float")
    got, _ = _got(negative_thr)
    assert np.isnan(got[sp == np.float32(-0.05)][0])  # not below -1: np.log10 of a negative value
    assert got[sp == np.float32(-1.0)][0] != np.float32(negative_thr.zerovalue) and np.isnan(got[sp == np.float32(-1.0)][0])
    assert got[np.isneginf(sp)][0] == np.float32(negative_thr.zerovalue)


@pytest.mark.parametrize("case", [c for c in CASES if c.R.size <= 4099], ids=lambda c: c.name)
def test_db_metadata_is_the_references(ref_pysteps, case):
    from pysteps.utils.transformation import dB_transform as ref_db

    _, want = _quiet(ref_db, case.R.copy(), case.metadata(), threshold=case.threshold, zerovalue=case.zerovalue,
                     inverse=case.inverse)
    assert _same_metadata(_got(case)[1], want), (_got(case)[1], want)


@pytest.mark.parametrize("form,thr", ew.threshold_forms(0.5) + [("none", None)])
def test_db_defaults_come_from_the_metadata(ref_pysteps, form, thr):
    """zerovalue=None and threshold=None, forwards and back: metadata as the reference's, values as the restatement's."""
    from pysteps.utils.transformation import dB_transform as ref_db
    from pysteps_amd.utils import dB_transform

    R = ew.quantised(0.16)
    meta = {"transform": None, "threshold": np.float32(0.16), "zerovalue": 0.0, "unit": "mm/h"}
    want, wmeta = ref_db(R.copy(), dict(meta), threshold=thr)
    dev, dmeta = dB_transform(_dev(R), dict(meta), threshold=thr)
    assert _same_metadata(dmeta, wmeta), (dmeta, wmeta)
    got = _host(dev)
    assert np.array_equal(got == np.float32(wmeta["zerovalue"]), want == np.float32(wmeta["zerovalue"]))
    back_w, bw = ref_db(want, wmeta, inverse=True)
    back_d, bd = dB_transform(_dev(want), dmeta, inverse=True)
    assert _same_metadata(bd, bw), (bd, bw)
    exp = ew.db_inverse(want, wmeta["threshold"], 0.0, ew.bar("inverse"))
    back = _host(back_d)
    assert np.array_equal((back == 0.0)[~exp.near], exp.zeros[~exp.near])
    same, again = dB_transform(dev, dmeta)  # already in dB: unchanged
    assert same is dev and again["transform"] == "dB"


# ---- dB inverse -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", INVERSE, ids=lambda c: c.name)
def test_db_inverse(case):
    got, _ = _got(case)
    bar = ew.bar("inverse") * case.bar_scale
    exp = ew.expectation(case, bar=bar)
    if case.name in ew.ISOLATING_WANT:
        # exp10f(0) is exactly 1, so the comparison with 10^(1e-9) is decided by the threshold's type alone
        assert got.tolist() == ew.ISOLATING_WANT[case.name], got.tolist()
        return
    zeroed = got == np.float32(case.zerovalue)
    decided = ~exp.near
    assert np.array_equal(zeroed[decided], exp.zeros[decided]), np.flatnonzero(decided & (zeroed != exp.zeros))[:8]
    # whatever was kept - the undecided elements too - is within the bar of its value
    dev, wrong = ew.deviation(got, exp.value, ~zeroed)
    print("inverse %-34s n=%-8d worst deviation %.3f spacings (bar %.2f), left open %d = %.2e of the case"
          % (case.name, case.R.size, dev, bar, np.count_nonzero(exp.near), exp.near_share()))
    assert wrong == 0
    assert dev <= bar, dev
    if case.continuous:
        assert exp.near_share() <= ew.NEAR_CAP, exp.near_share()
    elif case.kind == "roundtrip":
        # only the level that sits on the threshold, with its two neighbours, may be open
        assert np.count_nonzero(exp.near) <= 3, np.flatnonzero(exp.near)


def test_db_inverse_subnormal_results_are_kept():
    case = next(c for c in INVERSE if c.kind == "extreme")
    got, _ = _got(case)
    sub = got[case.R == np.float32(-400.0)][0]
    assert 0.0 < sub < np.float32(ew.FLT_MIN), sub
    assert np.isposinf(got[case.R == np.float32(390.0)][0])


# ---- position and alignment -------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_misaligned_planes_give_the_bits_of_an_aligned_copy(inverse):
    """Every view of the (3, 37, 53) stack - planes 1 and 2 start 4 and 8 bytes off 16-byte alignment - against the same
    plane uploaded on its own.  Device against device: no tolerance."""
    planes = [c for c in CASES if c.name.startswith("%s-stack-plane" % ("inv" if inverse else "fwd"))]
    assert len(planes) == ew.STACK_SHAPE[0]
    stack_dev = _dev(np.stack([c.R for c in planes]))
    for k, case in enumerate(planes):
        view = stack_dev.view(k)
        assert view.ptr % 16 == (k * case.R.size * 4) % 16 and (k == 0 or view.ptr % 16)
        got, _ = _transform(view, case)
        alone, _ = _got(case)
        assert _same_values(got, alone), (k, np.flatnonzero(_bits(got) != _bits(alone))[:8])
    # a misaligned destination alone (in place on an aligned source is the ordinary path): through the C entry point
    case = planes[1]
    dst = _dev(np.zeros((2, case.R.size), np.float32)).view(1)
    assert dst.ptr % 16
    src = _dev(case.R)
    thr = ew.compared_with(ew.inverse_threshold_lin(case.threshold) if inverse else case.threshold)
    lib_mod = _lib()
    lib_mod.check(lib_mod.lib().psh_db_transform_dev(src.ptr, dst.ptr, src.size, thr, float(case.zerovalue), int(inverse)),
                  "psh_db_transform_dev")
    assert _same_values(_host(dst), _got(case)[0].ravel())


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_grid_stride_gives_the_bits_of_a_short_run(inverse):
    big = next(c for c in CASES if c.inverse == inverse and c.R.size == ew.GRID_STRIDE)
    got, _ = _got(big)
    head = ew.Case("head", inverse, big.R[:4099].copy(), big.threshold, big.zerovalue, big.kind)
    alone, _ = _transform(_dev(head.R), head)
    assert _same_values(got[:4099], alone)
    # and the tail past the last whole float4, which other threads of the same launch write
    tail = ew.Case("tail", inverse, big.R[-7:].copy(), big.threshold, big.zerovalue, big.kind)
    assert _same_values(got[-7:], _transform(_dev(tail.R), tail)[0])


# ---- dtype ----------------------------------------------------------------------------------------------------------------


def test_float64_resident_fields_are_refused():
    from pysteps_amd.utils import dB_transform
    from pysteps_amd.utils.transformation import field_nanmin, field_stats

    wide = _dev(np.linspace(0.0, 30.0, 16, dtype=np.float64))
    assert wide.dtype == np.float64
    for call in (lambda: dB_transform(wide), lambda: dB_transform(wide, {"transform": "dB"}, inverse=True),
                 lambda: field_stats(wide), lambda: field_nanmin(wide)):
        with pytest.raises(ValueError, match="device-resident fields must be float32"):
            call()


# ---- reductions -----------------------------------------------------------------------------------------------------------


def _check_stats(field_dev, a):
    from pysteps_amd.utils.transformation import field_nanmin, field_stats

    want = ew.stats(a)
    mn, mx, bad = field_stats(field_dev)
    assert (mn, mx, bad) == (want["min_finite"], want["max_finite"], want["nonfinite"])
    assert isinstance(bad, int)
    assert _same_number(field_nanmin(field_dev), want["nanmin"])


@pytest.mark.parametrize("name,a", ew.stats_cases(), ids=[n for n, _ in ew.stats_cases()])
def test_field_stats(name, a):
    _check_stats(_dev(a), a)


def _misaligned_planes():
    planes = ew.stack() - np.float32(3.0)
    planes[1, 0, 0] = np.nan
    planes[1, -1, -1] = -np.inf  # the last element of a view that starts 4 bytes off
    planes[2, 0, 0] = np.inf
    planes[2, 17, 5] = np.nan
    return planes


def test_field_stats_on_misaligned_views():
    planes = _misaligned_planes()
    stack_dev = _dev(planes)
    for k in range(planes.shape[0]):
        _check_stats(stack_dev.view(k), planes[k])


def _norain_fields():
    x = np.float32(0.7)
    up = np.nextafter(x, np.float32(np.inf))
    out = []
    for k, n in enumerate(ew.SIZES + (ew.STATS_LOOP, ew.GRID_STRIDE)):
        a = ew.rates(n, 500 + k)
        a[::3] = x
        a[1::3] = up
        if n > 4:
            a[n // 2] = np.nan  # never counts
        out.append(("n%d" % n, a))
    low = out[-3][1].copy()
    low[-1] = -np.inf  # precip_thr=None: the minimum is -inf and everything else that is a number counts
    out.append(("ninf-n%d" % low.size, low))
    return out


def _norain_thresholds():
    x = np.float64(np.float32(0.7))
    step = np.float64(np.spacing(np.float32(0.7)))
    out = [("none", None)]
    # between float32(0.7) and the next float32: a quarter and three quarters of the way, so that rounding the
    # threshold to float32 first (Python float, numpy.float32) and comparing in float64 (numpy.float64) differ
    for frac in (0.25, 0.75):
        for form, thr in ew.threshold_forms(float(x + frac * step))[:3]:
            out.append(("%.2f-%s" % (frac, form), thr))
    out.append(("int1", 1))
    return out


def _check_norain_count(field_dev, a):
    """check_norain answers ``count / size <= norain_thr``; asking at count / size and at (count - 1) / size pins count."""
    from pysteps_amd.utils.check_norain import check_norain

    for label, thr in _norain_thresholds():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            count = int(np.count_nonzero(a > (np.nanmin(a) if thr is None else thr)))
        assert check_norain(field_dev, precip_thr=thr, norain_thr=count / a.size, printmsg=False), (label, count)
        if count:
            assert not check_norain(field_dev, precip_thr=thr, norain_thr=(count - 1) / a.size, printmsg=False), (label, count)


@pytest.mark.parametrize("name,a", _norain_fields(), ids=[n for n, _ in _norain_fields()])
def test_check_norain_counts_as_numpy(name, a):
    if a.size > 4:
        x, up = np.float64(np.float32(0.7)), np.float64(np.nextafter(np.float32(0.7), np.float32(np.inf)))
        step = up - x
        # the inputs do tell the threshold types apart
        assert np.count_nonzero(a > np.float64(x + 0.75 * step)) > np.count_nonzero(a > float(x + 0.75 * step))
        assert np.count_nonzero(a > np.float64(x + 0.25 * step)) == np.count_nonzero(a > float(x + 0.25 * step))
    _check_norain_count(_dev(a), a)


def test_check_norain_on_misaligned_views():
    planes = _misaligned_planes()
    planes[:, ::2, :] = np.float32(0.7)
    planes[:, 1::2, ::2] = np.nextafter(np.float32(0.7), np.float32(np.inf))
    planes[1, -1, -1] = -np.inf
    stack_dev = _dev(planes)
    for k in range(planes.shape[0]):
        _check_norain_count(stack_dev.view(k), planes[k])


def _nonfinite_f64(field_dev):
    count = ctypes.c_double(-1.0)
    lib_mod = _lib()
    lib_mod.check(lib_mod.lib().psh_nonfinite_count_f64_dev(field_dev.ptr, field_dev.size, ctypes.byref(count)),
                  "psh_nonfinite_count_f64_dev")
    return count.value


@pytest.mark.parametrize("name,a", ew.stats_cases(), ids=[n for n, _ in ew.stats_cases()])
def test_nonfinite_count_f64(name, a):
    wide = a.astype(np.float64)
    if wide.size > 2:
        wide[1] = 1e300  # finite, though beyond float32's range
        wide[2] = -1e-320  # a float64 subnormal
    assert _nonfinite_f64(_dev(wide)) == float(np.count_nonzero(~np.isfinite(wide)))


def test_nonfinite_count_f64_on_an_odd_offset():
    wide = _misaligned_planes().astype(np.float64)
    stack_dev = _dev(wide)
    for k in range(wide.shape[0]):
        assert _nonfinite_f64(stack_dev.view(k)) == float(np.count_nonzero(~np.isfinite(wide[k])))


# ---- resident outval="min" ------------------------------------------------------------------------------------------------


def test_resident_outval_min_is_nanmin(ref_pysteps):
    """A field that holds a -inf: the resident call equals the host call of this package bit for bit, and the host call
    fills what leaves the domain with np.nanmin, as the reference does (semilagrangian.py:171-172)."""
    from pysteps.extrapolation.semilagrangian import extrapolate as ref_extrapolate
    from pysteps_amd.extrapolation.semilagrangian import extrapolate

    m, n = 24, 32
    precip = ew.rates(m * n, 600).reshape(m, n)
    precip[5, 20] = -np.inf
    velocity = np.zeros((2, m, n), np.float32)
    velocity[0] = 2.5  # the three columns on the left come from outside the domain
    kw = dict(outval="min", allow_nonfinite_values=True)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = ref_extrapolate(precip, velocity, 2, **kw)
    host = extrapolate(precip, velocity, 2, **kw)
    resident = _host(extrapolate(_dev(precip), _dev(velocity), 2, **kw))
    assert np.nanmin(precip) == -np.inf
    assert np.all(np.isneginf(want[0][:, :2])) and np.all(np.isneginf(host[0][:, :2]))
    assert host.dtype == np.float32 and _same_values(resident, host), np.argwhere(_bits(resident) != _bits(host))[:8]
    assert np.array_equal(np.isneginf(host), np.isneginf(want))


# ---- psh_convert_dev ------------------------------------------------------------------------------------------------------


def _convert(src, to_f64):
    from pysteps_amd.device import DeviceArray

    src_dev = _dev(src)
    out = DeviceArray(src.shape, np.float64 if to_f64 else np.float32)
    lib_mod = _lib()
    lib_mod.check(lib_mod.lib().psh_convert_dev(src_dev.ptr, out.ptr, src.size, int(to_f64)), "psh_convert_dev")
    got = _host(out)
    src_dev.free()
    out.free()
    return got


def _tiled(pattern, n):
    return np.resize(pattern, n)  # repeats the pattern; a size that is no multiple of it ends part-way through


@pytest.mark.parametrize("n", ew.SIZES + (ew.STATS_LOOP, ew.GRID_STRIDE))
def test_convert_equals_astype(n):
    wide = _tiled(ew.wide_pattern(), n)
    with np.errstate(over="ignore"):
        want = wide.astype(np.float32)
    assert _same_values(_convert(wide, False), want)
    narrow = _tiled(ew.narrow_pattern(), n)
    assert _same_values(_convert(narrow, True), narrow.astype(np.float64))


def test_convert_past_the_block_cap():
    """2^26 + 3 elements: the first size at which the launch's 65 535-block cap makes the stride loop run."""
    n = (1 << 26) + 3
    wide = _tiled(ew.wide_pattern(), n)
    with np.errstate(over="ignore"):
        want = wide.astype(np.float32)
    got = _convert(wide, False)
    del wide
    assert got.dtype == np.float32 and np.array_equal(np.isnan(got), np.isnan(want))
    keep = ~np.isnan(want)
    assert np.array_equal(_bits(got)[keep], _bits(want)[keep])
    del got, keep
    narrow = _tiled(ew.narrow_pattern(), n)
    back = _convert(narrow, True)
    want = narrow.astype(np.float64)
    keep = ~np.isnan(want)
    assert np.array_equal(np.isnan(back), ~keep) and np.array_equal(_bits(back)[keep], _bits(want)[keep])


# ---- psh_axpy_f64_dev -----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("alpha", [1.0, -1.0, 0.5, 2.0])
def test_axpy_f64_equals_numpy(alpha):
    """alpha x src is exact for these alphas, so a fused and an unfused evaluation agree: bit for bit with NumPy."""
    lib_mod = _lib()
    for k, n in enumerate((1, 2, 3, 5, 1023, 4099, 1_100_003)):  # the last: more than 256 CUs x 16 blocks x 256 threads
        rng = np.random.default_rng(800 + k)
        dst = rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 8, n)
        src = rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 8, n)
        specials = [(0.0, 0.0), (-0.0, 0.0), (-0.0, -0.0), (0.0, -0.0), (np.inf, 1.0), (1.0, -np.inf), (np.inf, np.inf),
                    (np.inf, -np.inf), (np.nan, 1.0), (1.0, np.nan), (1.0, -1.0), (1e308, 1e308), (0.1, 0.2)]
        for j, (d, s) in enumerate(specials[:n]):
            dst[-1 - j], src[-1 - j] = d, s  # at the end: the tail of the launch
        with np.errstate(all="ignore"):
            want = dst + alpha * src
        dst_dev, src_dev = _dev(dst), _dev(src)
        lib_mod.check(lib_mod.lib().psh_axpy_f64_dev(dst_dev.ptr, src_dev.ptr, alpha, n), "psh_axpy_f64_dev")
        assert _same_values(_host(dst_dev), want), (n, alpha)
        assert _same_values(_host(src_dev), src)
