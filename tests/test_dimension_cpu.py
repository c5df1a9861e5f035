"""``pysteps_amd.utils.dimension`` on host arrays, and the restatement of tests/helpers/dimension.py, against
tests/golden/dimension_reference.npz (written by the unmodified reference, tools/make_golden_dimension.py).  No GPU.

Comparison is helpers.dimension.mismatch: shapes, dtypes, NaN masks, and the bits of every element that is not NaN."""

import json
import warnings

import numpy as np
import pytest

from helpers import dimension as hd

GOLD = hd.load_golden()
FUNCTIONS = ("aggregate_fields", "aggregate_fields_time", "aggregate_fields_space", "clip_domain", "square_domain")


def _quiet(fn, *args, **kwargs):
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*args, **kwargs)


def _call(call, x):
    from pysteps_amd.utils import dimension

    meta = hd.golden_meta(call)
    args = (x,) if meta is None else (x, meta)
    return _quiet(getattr(dimension, call["fn"]), *args, **hd.golden_kwargs(call)), meta


@pytest.mark.parametrize("fn", FUNCTIONS)
def test_host_path_gives_the_references_arrays_and_metadata(fn):
    calls = hd.golden_calls(GOLD, fn)
    assert len(calls) >= 10
    for call in calls:
        x = GOLD[call["x"]]
        before = x.copy()
        res, meta_in = _call(call, x)
        if call["returns"] == "pair":
            assert isinstance(res, tuple) and len(res) == 2, call["id"]
            res, meta_out = res
            assert hd.same_meta(meta_out, hd.decode_meta(str(GOLD[call["id"] + "/meta_out"]))), call["id"]
            assert hd.same_meta(meta_in, hd.decode_meta(call["meta"])), call["id"]  # the caller's dictionary is left alone
        assert isinstance(res, np.ndarray), call["id"]
        assert hd.mismatch(res, GOLD[call["id"] + "/out"]) is None, (call["id"], hd.mismatch(res, GOLD[call["id"] + "/out"]))
        assert hd.mismatch(x, before) is None and not np.shares_memory(res, x), call["id"]


def test_restatement_gives_the_references_aggregates():
    seen = 0
    for call in hd.golden_calls(GOLD, "aggregate_fields"):
        kw = hd.golden_kwargs(call)
        if not np.isscalar(kw["axis"]):
            continue
        got = _quiet(hd.aggregate, GOLD[call["x"]], kw["window_size"], kw["axis"], kw["method"], kw["trim"])
        assert hd.mismatch(got, GOLD[call["id"] + "/out"]) is None, (call["id"], hd.mismatch(got, GOLD[call["id"] + "/out"]))
        seen += 1
    assert seen == 13 * 2 * 4
    for call in hd.golden_calls(GOLD, "aggregate_fields_space"):
        kw = hd.golden_kwargs(call)
        if kw["space_window"] is None or kw["space_window"] == 1.0:
            continue
        wx, wy = (kw["space_window"],) * 2 if np.isscalar(kw["space_window"]) else kw["space_window"]
        got = _quiet(hd.upscale, GOLD[call["x"]], int(wy), int(wx), kw["ignore_nan"])
        assert hd.mismatch(got, GOLD[call["id"] + "/out"]) is None, (call["id"], hd.mismatch(got, GOLD[call["id"] + "/out"]))


def test_golden_inputs_tell_summation_orders_apart():
    """Recorded when the file was written: for every aggregate case with a window of 3 or more, a reversed-order sum and a
    pairwise sum each differ from the reference on at least one element.  Checked again here on the stored inputs."""
    check = json.loads(str(GOLD["order_check"]))
    wide = {c["x"].split("/")[0] for c in hd.golden_calls(GOLD, "aggregate_fields")
            if np.isscalar(c["kwargs"]["axis"]) and c["kwargs"]["window_size"] >= 3}
    assert set(check) == wide and len(wide) >= 16
    for tag, row in check.items():
        assert row["reversed_differs_on"] >= 1 and row["pairwise_differs_on"] >= 1, tag
        call = next(c for c in hd.golden_calls(GOLD, "aggregate_fields") if c["id"] == tag + "_nansum")
        back, tree = _quiet(hd.reordered_sums, GOLD[call["x"]], call["kwargs"]["window_size"], call["kwargs"]["axis"])
        want = GOLD[call["id"] + "/out"]
        assert np.count_nonzero(hd.bits(back) != hd.bits(want)) == row["reversed_differs_on"], tag
        assert np.count_nonzero(hd.bits(tree) != hd.bits(want)) == row["pairwise_differs_on"], tag


def test_exceptions_have_the_references_types_and_texts():
    from pysteps_amd.utils import dimension

    errors = json.loads(str(GOLD["errors"]))
    bad = hd.bad_calls()
    assert sorted(errors) == sorted(cid for cid, _, _, _ in bad) and len(bad) >= 20
    for cid, fn, args, kwargs in bad:
        with pytest.raises(Exception) as info:
            getattr(dimension, fn)(*args, **kwargs)
        assert [type(info.value).__name__, str(info.value)] == errors[cid], cid


def test_early_returns_hand_back_copies():
    from pysteps_amd.utils import dimension

    x = hd.rain((6, 9, 11), 5, np.float32)
    meta = dict(hd.geo(9, 11), timestamps=hd.stamps(6))
    for res, out_meta in (dimension.aggregate_fields_time(x, meta, None), dimension.aggregate_fields_time(x, meta, 5),
                          dimension.aggregate_fields_space(x, meta, None), dimension.aggregate_fields_space(x, meta, 1.0),
                          dimension.clip_domain(x, meta, None)):
        assert hd.mismatch(res, x) is None and not np.shares_memory(res, x)
        assert out_meta == meta and out_meta is not meta


def test_square_domain_keeps_the_references_habits():
    from pysteps_amd.utils import dimension

    # an already square field: squeezed, and alone
    x = hd.rain((1, 8, 8), 6, np.float32)
    res = dimension.square_domain(x, hd.geo(8, 8))
    assert isinstance(res, np.ndarray) and res.shape == (8, 8) and hd.mismatch(res, x[0]) is None
    # the inverse takes its two keys out of the metadata it returns, not out of the caller's
    y = hd.rain((12, 20), 7, np.float64, 0.0)
    padded, meta = dimension.square_domain(y, hd.geo(12, 20), method="pad")
    assert padded.shape == (20, 20) and meta["orig_domain"] == (12, 20) and meta["square_method"] == "pad"
    back, meta_back = dimension.square_domain(padded, meta, inverse=True)
    assert hd.mismatch(back, y) is None
    assert "orig_domain" not in meta_back and "square_method" not in meta_back and "orig_domain" in meta
    assert {k: meta_back[k] for k in ("x1", "x2", "y1", "y2")} == {k: hd.geo(12, 20)[k] for k in ("x1", "x2", "y1", "y2")}
    # any NaN makes the pad value NaN
    y[3, 4] = np.nan
    padded, _ = dimension.square_domain(y, hd.geo(12, 20), method="pad")
    assert np.isnan(padded[:4]).all() and np.isnan(padded[-4:]).all()


def test_dtype_keyword_stores_the_requested_type():
    from pysteps_amd.utils import dimension

    x = hd.rain((3, 12, 20), 8, np.float64)
    meta = hd.geo(12, 20)
    wide, _ = dimension.clip_domain(x, meta, (-3, 10, 2, 9))
    narrow, _ = dimension.clip_domain(x, meta, (-3, 10, 2, 9), dtype=np.float32)
    assert wide.dtype == np.float64 and hd.mismatch(narrow, wide.astype(np.float32)) is None
    for method in ("pad", "crop"):
        wide, _ = dimension.square_domain(x, meta, method=method)
        narrow, _ = dimension.square_domain(x, meta, method=method, dtype=np.float32)
        assert wide.dtype == np.float64 and hd.mismatch(narrow, wide.astype(np.float32)) is None
    crop32, _ = dimension.square_domain(x.astype(np.float32), meta, method="crop")
    assert crop32.dtype == np.float32  # a slice keeps the dtype


def test_get_method_serves_the_dimension_names_from_this_package():
    from pysteps_amd import utils
    from pysteps_amd.utils import dimension

    assert utils.get_method("accumulate") is dimension.aggregate_fields_time
    assert utils.get_method("clip") is dimension.clip_domain
    assert utils.get_method("square") is dimension.square_domain
    assert utils.get_method("upscale") is dimension.aggregate_fields_space
    assert utils.get_method("Upscale") is dimension.aggregate_fields_space
    for name in ("aggregate_fields", "aggregate_fields_time", "aggregate_fields_space", "clip_domain", "square_domain"):
        assert getattr(utils, name) is getattr(dimension, name)


class Collector:
    def __init__(self):
        self.blocks = []

    def __call__(self, block):
        self.blocks.append(block)


@pytest.mark.parametrize("method", hd.METHODS)
@pytest.mark.parametrize("leadtimes, nframes", [(6, 2), (6, 3), (7, 3)])
def test_time_aggregator_on_host_arrays(method, leadtimes, nframes):
    """Frames added as they arrive equal aggregate_fields of the stacked block: widened to float64 by default, in float32
    with dtype=np.float32; an incomplete last window is dropped and counted."""
    from pysteps_amd.utils import dimension

    stack = hd.field((leadtimes, 3, 16, 24), 0, nframes, 900 + leadtimes, np.float32)
    complete = (leadtimes // nframes) * nframes
    for dtype in (None, np.float32):
        then = Collector()
        agg = dimension.TimeAggregator(nframes, method=method, then=then, dtype=dtype)
        for t in range(leadtimes):
            _quiet(agg, stack[t])
        block = stack[:complete] if dtype is not None else stack[:complete].astype(np.float64)
        want = _quiet(dimension.aggregate_fields, block, nframes, axis=0, method=method)
        assert agg.pending == leadtimes - complete and agg.n_windows == complete // nframes == len(then.blocks)
        assert hd.mismatch(np.stack(agg.fields), want) is None, hd.mismatch(np.stack(agg.fields), want)
        assert hd.mismatch(np.stack(then.blocks), want) is None
        assert agg.received == [np.ndarray] * leadtimes


def test_time_aggregator_arguments():
    from pysteps_amd.utils import dimension

    with pytest.raises(ValueError):
        dimension.TimeAggregator(3, method="median")
    with pytest.raises(ValueError):
        dimension.TimeAggregator(0)
    with pytest.raises(ValueError):
        dimension.TimeAggregator(3, keep="disk")
    with pytest.raises(ValueError):
        dimension.TimeAggregator(2, dtype=np.float32)(np.zeros((3, 4, 5)))  # float64 members into a float32 sum
    assert dimension.TimeAggregator.accepts_device
