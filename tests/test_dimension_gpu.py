"""``pysteps_amd.utils.dimension`` on resident fields (csrc/dimension.hip) against tests/golden/dimension_reference.npz
(written by the unmodified reference) and, for the shapes the file does not hold, against the NumPy restatement of
tests/helpers/dimension.py, which tests/test_dimension_cpu.py holds to the same file.

Comparison is helpers.dimension.mismatch throughout: equal shapes and dtypes, equal NaN masks, equal bits on every
element that is not NaN.  There is no tolerance anywhere, except in the RainFARM round trip at the end, which takes the
bar tests/test_rainfarm_gpu.py uses for the same property."""

import functools
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from helpers import dimension as hd

pytestmark = pytest.mark.gpu

GOLD = hd.load_golden()


def _dev(a):
    from pysteps_amd.device import DeviceArray

    return DeviceArray.from_host(np.ascontiguousarray(a))


def _host(d):
    from pysteps_amd.device import DeviceArray

    assert isinstance(d, DeviceArray), type(d)
    return d.to_host(out=np.empty(d.shape, d.dtype))


def _quiet(fn, *args, **kwargs):
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*args, **kwargs)


def _same(got, want, what):
    problem = hd.mismatch(got, want)
    assert problem is None, "%s: %s" % (what, problem)


@functools.lru_cache(maxsize=None)
def _field(shape, axis, w, seed, dtype):
    x = hd.field(shape, axis, w, seed, dtype)
    x.setflags(write=False)
    return x


# ---- the recorded calls of the reference, on the device ---------------------------------------------------------------------
@pytest.mark.parametrize("fn", ["aggregate_fields", "aggregate_fields_time", "aggregate_fields_space", "clip_domain", "square_domain"])
def test_recorded_calls_on_resident_fields(fn):
    """DeviceArray in, DeviceArray out, the reference's bits and metadata.  clip_domain: both origins, an extent inside
    the domain, one over an edge, one larger than the domain, (m, n) to (l, t, m, n).  square_domain: pad and crop of
    (12, 20), (3, 21, 12) (an odd difference) and (2, 2, 12, 19), a pad of a field with NaN (NaN fill), both inverses."""
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.utils import dimension

    calls = hd.golden_calls(GOLD, fn)
    assert len(calls) >= 10
    for call in calls:
        meta = hd.golden_meta(call)
        x = _dev(GOLD[call["x"]])
        args = (x,) if meta is None else (x, meta)
        res = _quiet(getattr(dimension, fn), *args, **hd.golden_kwargs(call))
        if call["returns"] == "pair":
            res, meta_out = res
            assert hd.same_meta(meta_out, hd.decode_meta(str(GOLD[call["id"] + "/meta_out"]))), call["id"]
            assert hd.same_meta(meta, hd.decode_meta(call["meta"])), call["id"]
        assert isinstance(res, DeviceArray) and res.ptr != x.ptr, call["id"]
        _same(_host(res), GOLD[call["id"] + "/out"], call["id"])
        _same(_host(x), GOLD[call["x"]], call["id"] + " (input left alone)")


# ---- the axis kernel ------------------------------------------------------------------------------------------------------------
AXIS_CASES = (
    [((6, 5, 7), axis, w) for axis in range(3) for w in (1, 2, 3, 5, 6) if w <= (6, 5, 7)[axis]]
    + [((6, 5, 7), axis, 4) for axis in range(3)]
    + [((2, 3, 12, 20), 1, 3), ((2, 3, 12, 20), 2, 4), ((2, 3, 12, 20), 2, 12), ((2, 3, 12, 20), 3, 5), ((2, 3, 12, 20), 3, 20)]
    + [((3, 37, 61), 2, 3), ((3, 37, 61), 1, 3)]              # odd rows; post == 1 with a window that is no power of two
    + [((2, 9, 710), 2, w) for w in (2, 5, 71, 710)]          # rows off the 16-byte boundary, a window wider than a wave
    + [((1300, 3), 0, 650), ((1300, 3), 0, 2)]                # a long window with a small post
    + [((2, 600, 8), 1, 300), ((520, 64), 1, 4), ((520, 64), 1, 32), ((520, 64), 1, 64)]  # vector paths, chunked windows
)


@pytest.mark.parametrize("method", hd.METHODS)
@pytest.mark.parametrize("dtype", hd.DTYPES, ids=["float32", "float64"])
def test_aggregate_fields_along_one_axis(dtype, method):
    from pysteps_amd.utils import dimension

    for number, (shape, axis, w) in enumerate(AXIS_CASES):
        x = _field(shape, axis, w, 700 + number, dtype)
        trim = shape[axis] % w != 0
        got = _host(dimension.aggregate_fields(_dev(x), w, axis=axis, method=method, trim=trim))
        _same(got, _quiet(hd.aggregate, x, w, axis, method, trim), "%s axis %d window %d" % (shape, axis, w))


@pytest.mark.parametrize("method", hd.METHODS)
def test_aggregate_a_plane_that_starts_off_the_16_byte_boundary(method):
    """stack.view(1) of (2, 33, 61) float32 planes: 8052 bytes into the allocation."""
    from pysteps_amd.utils import dimension

    stack = _field((2, 33, 61), 1, 3, 750, np.float32)
    plane = _dev(stack).view(1)
    assert plane.ptr % 16 == 4
    for axis, w, trim in ((0, 3, False), (0, 11, False), (1, 4, True), (1, 61, False)):
        got = _host(dimension.aggregate_fields(plane, w, axis=axis, method=method, trim=trim))
        _same(got, _quiet(hd.aggregate, stack[1], w, axis, method, trim), "axis %d window %d" % (axis, w))
    wide = _dev(stack.astype(np.float64)).view(1)
    got = _host(dimension.aggregate_fields(wide, 3, axis=0, method=method))
    _same(got, _quiet(hd.aggregate, stack[1].astype(np.float64), 3, 0, method), "float64 view")


def test_tuple_axes_recurse():
    from pysteps_amd.utils import dimension

    x = _field((2, 3, 12, 20), 2, 4, 760, np.float32)
    got = _host(dimension.aggregate_fields(_dev(x), (4, 5), axis=(2, 3), method="nanmean"))
    _same(got, _quiet(hd.upscale, x, 4, 5, True), "tuple")


def test_the_pairwise_case_and_other_dtypes_are_refused():
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.utils import dimension

    line = _dev(np.arange(64, dtype=np.float32))
    with pytest.raises(NotImplementedError, match="pairwise"):
        dimension.aggregate_fields(line, 8)
    with pytest.raises(NotImplementedError, match="pairwise"):
        dimension.aggregate_fields(_dev(np.zeros((1, 16, 1))), 16, axis=1)
    got = _host(dimension.aggregate_fields(line, 4, method="sum"))  # below 8 entries NumPy adds in order
    _same(got, np.arange(64, dtype=np.float32).reshape(16, 4).sum(axis=1), "short windows of a line")
    ints = DeviceArray((4, 6), np.int32)
    with pytest.raises(NotImplementedError, match="float32 or float64"):
        dimension.aggregate_fields(ints, 2)
    with pytest.raises(NotImplementedError):
        dimension.clip_domain(ints, hd.geo(4, 6), (1, 3, 1, 3))
    with pytest.raises(ValueError, match="must exactly divide"):
        dimension.aggregate_fields(_dev(np.zeros((5, 4), np.float32)), 2)


# ---- the upscale ----------------------------------------------------------------------------------------------------------------
SPACE_CASES = [((12, 20), 4, 5), ((3, 12, 20), 4, 5), ((3, 12, 20), 12, 20), ((2, 3, 12, 20), 4, 5), ((2, 3, 12, 20), 12, 20),
               ((130, 192), 65, 64), ((2, 130, 192), 130, 96),  # beyond the fused kernel: two launches
               ((64, 128), 2, 2), ((3, 64, 132), 64, 3), ((2, 37, 61), 37, 1), ((5, 1100), 1, 2), ((128, 2112), 64, 64)]


@pytest.mark.parametrize("ignore_nan", [False, True])
@pytest.mark.parametrize("dtype", hd.DTYPES, ids=["float32", "float64"])
def test_aggregate_fields_space(dtype, ignore_nan):
    from pysteps_amd.utils import dimension

    for number, (shape, wy, wx) in enumerate(SPACE_CASES):
        x = hd.field_space(shape, wy, wx, 800 + number, dtype)
        meta = hd.geo(*shape[-2:])
        got, meta_out = dimension.aggregate_fields_space(_dev(x), meta, (wx, wy), ignore_nan=ignore_nan)
        _same(_host(got), _quiet(hd.upscale, x, wy, wx, ignore_nan), "%s by (%d, %d)" % (shape, wy, wx))
        assert meta_out["ypixelsize"] == wy and meta_out["xpixelsize"] == wx and meta["xpixelsize"] == 1.0


@pytest.mark.parametrize("dtype", hd.DTYPES, ids=["float32", "float64"])
def test_fused_and_two_launch_routes_give_the_same_bits(dtype):
    from pysteps_amd.utils import dimension

    for shape, wy, wx in (((3, 64, 128), 2, 2), ((2, 36, 60), 4, 5), ((128, 128), 64, 64)):
        x = _dev(hd.field_space(shape, wy, wx, 850, dtype))
        axes = [len(shape) - 2, len(shape) - 1]
        for method in ("mean", "nanmean"):
            fused = _host(dimension._upscale_dev(x, axes, [wy, wx], method, route="fused"))
            two = _host(dimension._upscale_dev(x, axes, [wy, wx], method, route="two_launch"))
            _same(fused, two, "%s by (%d, %d) %s" % (shape, wy, wx, method))
    # (130, 192) by (130, 96) as ONE plane: the x pass reduces a single row, which NumPy sums pairwise (the reference's
    # result there is not the in-order sum) - the case the device declines; with a leading axis it is served (SPACE_CASES)
    with pytest.raises(NotImplementedError, match="pairwise"):
        dimension.aggregate_fields_space(_dev(np.zeros((130, 192), dtype)), hd.geo(130, 192), (96, 130))
    with pytest.raises(ValueError, match="fused"):
        dimension._upscale_dev(_dev(np.zeros((130, 192), dtype)), [0, 1], [65, 64], "mean", route="fused")


# ---- clip and square --------------------------------------------------------------------------------------------------------------
def test_dtype_keyword_on_resident_fields():
    """dtype=np.float32 stores float32; the host path (held to the reference by test_dimension_cpu.py) is the yardstick."""
    from pysteps_amd.utils import dimension

    for dtype in hd.DTYPES:
        x = hd.rain((3, 12, 20), 860, dtype)
        meta = hd.geo(12, 20)
        for extent in ((4, 15, 2, 9), (-3, 10, 2, 9), (-2, 23, -3, 14)):
            want, want_meta = dimension.clip_domain(x, meta, extent, dtype=np.float32)
            got, got_meta = dimension.clip_domain(_dev(x), meta, extent, dtype=np.float32)
            _same(_host(got), want, "clip %s" % (extent,))
            assert got_meta == want_meta and want.dtype == np.float32
        for method in ("pad", "crop"):
            want, want_meta = dimension.square_domain(x, meta, method=method, dtype=np.float32)
            got, got_meta = dimension.square_domain(_dev(x), meta, method=method, dtype=np.float32)
            _same(_host(got), want, "square %s" % method)
            assert got_meta == want_meta
            back, back_meta = dimension.square_domain(got, got_meta, inverse=True, dtype=np.float32)
            want_back, want_back_meta = dimension.square_domain(want, want_meta, inverse=True, dtype=np.float32)
            _same(_host(back), want_back, "inverse of %s" % method)
            assert back_meta == want_back_meta


def test_square_domain_round_trip_and_habits():
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.utils import dimension

    x = hd.rain((3, 21, 12), 870, np.float32, 0.0)
    meta = hd.geo(21, 12)
    padded, pmeta = dimension.square_domain(_dev(x), meta, method="pad")
    assert padded.shape == (3, 21, 21) and padded.dtype == np.float64 and pmeta["orig_domain"] == (21, 12)
    back, bmeta = dimension.square_domain(padded, pmeta, inverse=True)
    _same(_host(back), x.astype(np.float64), "pad, then its inverse")
    assert "orig_domain" not in bmeta and "square_method" not in bmeta and "orig_domain" in pmeta
    assert {k: bmeta[k] for k in ("x1", "x2", "y1", "y2")} == {k: meta[k] for k in ("x1", "x2", "y1", "y2")}
    x[1, 5, 5] = np.nan  # any NaN makes the fill NaN
    padded, _ = dimension.square_domain(_dev(x), meta, method="pad")
    got = _host(padded)
    assert np.isnan(got[:, :, :4]).all() and np.isnan(got[:, :, -5:]).all()
    _same(got[:, :, 4:16], x.astype(np.float64), "the field inside a NaN frame")
    square = dimension.square_domain(_dev(x[:, :12, :]), hd.geo(12, 12))  # already square: the array alone
    assert isinstance(square, DeviceArray) and square.shape == (3, 12, 12)
    _same(_host(square), x[:, :12, :], "already square")


# ---- the running accumulator ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _leadtimes(count, nframes):
    x = hd.field((count, 3, 16, 24), 0, nframes, 900 + count, np.float32)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("method", hd.METHODS)
@pytest.mark.parametrize("leadtimes, nframes", [(6, 2), (6, 3), (7, 3)])
def test_time_aggregator_on_resident_members(method, leadtimes, nframes):
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.utils import dimension

    stack = _leadtimes(leadtimes, nframes)
    complete = (leadtimes // nframes) * nframes
    meta = {"unit": "mm/h" if "mean" in method else "mm", "timestamps": hd.stamps(complete), "accutime": 5}
    for dtype in (None, np.float32):
        for keep in ("host", "device"):
            agg = dimension.TimeAggregator(nframes, method=method, keep=keep, dtype=dtype)
            members = _dev(stack)
            for t in range(leadtimes):
                agg(members.view(t))
            block = stack[:complete] if dtype is not None else stack[:complete].astype(np.float64)
            want = _quiet(hd.aggregate, block, nframes, 0, method)
            # ... which is aggregate_fields_time of the stacked block, members as the leading axis
            ref, _ = dimension.aggregate_fields_time(_dev(np.ascontiguousarray(block.swapaxes(0, 1))), meta, 5 * nframes,
                                                     ignore_nan=method.startswith("nan"))
            _same(_host(ref), np.ascontiguousarray(want.swapaxes(0, 1)), "aggregate_fields_time")
            got = agg.fields if keep == "host" else [_host(f) for f in agg.fields]
            _same(np.stack(got), want, "%s keep=%s dtype=%s" % (method, keep, dtype))
            assert agg.pending == leadtimes - complete and agg.received == [DeviceArray] * leadtimes


def test_time_aggregator_feeds_ensemble_products_on_the_device():
    from pysteps_amd.device import DeviceArray
    from pysteps_amd.postprocessing import ensemblestats
    from pysteps_amd.utils import dimension

    stack = _leadtimes(6, 3)
    products = ensemblestats.EnsembleProducts([0.5, 2.0])
    agg = dimension.TimeAggregator(3, method="nansum", then=products)
    members = _dev(stack)
    for t in range(6):
        agg(members.view(t))
    assert products.received == [DeviceArray] * 2 and agg.n_windows == 2
    blocks = _quiet(hd.aggregate, stack.astype(np.float64), 3, 0, "nansum")
    _same(np.stack(agg.fields), blocks, "blocks")
    for i in range(2):
        _same(products.excprob[i], ensemblestats.excprob(blocks[i], [0.5, 2.0]), "excprob of window %d" % i)
        _same(products.mean[i], ensemblestats.mean(blocks[i]), "mean of window %d" % i)


# ---- the same input, the same bits ------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_call_or_the_position_in_a_stack():
    from pysteps_amd.utils import dimension

    plane = hd.field_space((33, 63), 11, 3, 950, np.float32)
    stack = np.stack([hd.rain((33, 63), 951, np.float32), plane, plane])
    meta = hd.geo(33, 63)
    alone = _dev(plane)
    first = _host(dimension.aggregate_fields_space(alone, meta, (3, 11), ignore_nan=True)[0])
    again = _host(dimension.aggregate_fields_space(alone, meta, (3, 11), ignore_nan=True)[0])
    whole = _host(dimension.aggregate_fields_space(_dev(stack), meta, (3, 11), ignore_nan=True)[0])
    off = _host(dimension.aggregate_fields_space(_dev(stack).view(1), meta, (3, 11), ignore_nan=True)[0])  # off the 16-byte boundary
    for other, what in ((again, "second call"), (whole[1], "plane 1 of a stack"), (whole[2], "plane 2"), (off, "a view")):
        _same(other, first, what)
    for axis, w in ((0, 11), (1, 7)):
        a = _host(dimension.aggregate_fields(alone, w, axis=axis, method="nanmean"))
        b = _host(dimension.aggregate_fields(_dev(stack), w, axis=axis + 1, method="nanmean"))
        _same(b[1], a, "axis %d in a stack" % axis)
        _same(b[2], a, "axis %d in a stack" % axis)


# ---- after psh_shutdown ---------------------------------------------------------------------------------------------------------
def test_entry_points_answer_not_initialised_after_shutdown():
    """A child process: psh_init, one aggregation, psh_shutdown, then every entry point of csrc/dimension.hip with zero
    arguments - PSH_ENOTINIT, as tests/test_dimension_capi_cpu.py records for a library that was never initialised."""
    from test_dimension_capi_cpu import EXPECTED

    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "dimension_entry.py")
    run = subprocess.run([sys.executable, script, "--after-shutdown"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
    assert json.loads(run.stdout.strip().split("\n")[-1]) == EXPECTED


# ---- downscale, then upscale ------------------------------------------------------------------------------------------------------
def test_upscaling_a_rainfarm_field_returns_its_coarse_input():
    """rainfarm_hip without a smoothing kernel keeps the block means; aggregate_fields_space has to find them again.  Bar:
    the one tests/test_rainfarm_gpu.py::test_finish_stage holds the same property to - 5 x the golden file's
    deviation_finish, relative to the largest value of the fine field."""
    from helpers import rainfarm as rf

    from pysteps_amd.downscaling.rainfarm import downscale
    from pysteps_amd.utils import dimension

    precip = rf.field((16, 16), 108)
    fine = downscale(_dev(precip), 4, alpha=1.5, kernel_type=None, randstate=np.random.RandomState(108))
    assert fine.shape == (64, 64) and fine.dtype == np.float64
    meta = hd.geo(64, 64)
    coarse, meta_out = dimension.aggregate_fields_space(fine, meta, 4.0)
    got = _host(coarse)
    assert got.shape == (16, 16) and np.isfinite(got).all() and meta_out["xpixelsize"] == 4.0
    bar = rf.BAR_FACTOR * float(rf.load_golden()["deviation_finish"])
    off = float(np.abs(got - precip).max() / np.abs(_host(fine)).max())
    print("block means of the downscaled field vs its input: %.3g (bar %.3g)" % (off, bar))
    assert off <= bar
