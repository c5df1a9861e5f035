"""Aggregation, clipping and squaring (pysteps_amd/utils/dimension.py): inputs, a NumPy restatement of the aggregation
that spells the order out, the comparison, and the reading of tests/golden/dimension_reference.npz.

The golden file is written by tools/make_golden_dimension.py from the unmodified reference; tests/test_dimension_cpu.py
holds :func:`aggregate` and the package's host path to it.  On the GPU machine, where the reference does not exist, the
restatement serves the shapes the golden file does not hold.

Comparison (:func:`mismatch`): equal shapes and dtypes, equal NaN masks, equal bits on every element that is not NaN -
signed zeros count, NaN sign and payload do not (the host's 0 / 0 carries a sign bit).  No tolerance.
"""

import datetime
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "dimension_reference.npz")
METHODS = ("sum", "mean", "nansum", "nanmean")
DTYPES = (np.float32, np.float64)


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def rain(shape, seed, dtype, nan_share=0.25):
    """About 60 % zeros, the rest gamma x 10**uniform(-3, 3) with full mantissas in ``dtype`` - sums of such values round
    at every step, so another order gives other bits - and ``nan_share`` NaN."""
    rng = np.random.default_rng(seed)
    x = rng.gamma(0.6, 4.0, size=shape) * 10.0 ** rng.uniform(-3.0, 3.0, size=shape)
    x[rng.random(shape) < 0.6] = 0.0
    x = x.astype(dtype)
    x[rng.random(shape) < nan_share] = np.nan
    return x


def field(shape, axis, w, seed, dtype, nan_share=0.25):
    """:func:`rain` of ``shape`` with the hard windows of an aggregation along ``axis`` by ``w`` written in: a window of NaN
    only, +inf and -inf in one window, a window of -0.0, a window of -0.0 with one NaN, a line of subnormals."""
    shape = tuple(shape)
    axis %= len(shape)
    n, rest = shape[axis], shape[:axis] + shape[axis + 1:]
    P = int(np.prod(rest, dtype=np.int64))
    v = rain((n, P), seed, dtype, nan_share)
    K = n // w
    if K >= 1:
        last = (K - 1) * w
        tiny = np.finfo(dtype).smallest_subnormal
        v[:, 4 % P] = tiny * np.random.default_rng(seed + 1).integers(1, 1000, size=n).astype(dtype)
        v[last:last + w, 3 % P] = -0.0
        if w > 1:
            v[last + w - 1, 3 % P] = np.nan
        v[0:w, 2 % P] = -0.0
        v[last, 1 % P] = np.inf
        if w > 1:
            v[last + 1, 1 % P] = -np.inf
        v[0:w, 0] = np.nan
    return np.ascontiguousarray(np.moveaxis(v.reshape((n,) + rest), 0, axis))


def field_space(shape, wy, wx, seed, dtype, nan_share=0.25):
    """:func:`rain` with the hard cells of an upscale by (wy, wx) of the last two axes: a cell of NaN only, one whose first
    column is NaN only (the y pass gives NaN, the x pass has to skip it), +inf and -inf in one cell, a cell of -0.0."""
    x = rain(tuple(shape), seed, dtype, nan_share)
    m, n = shape[-2:]
    ky, kx = m // wy, n // wx
    x[..., 0:wy, 0:wx] = np.nan
    cy, cx = (ky - 1) * wy, (kx - 1) * wx
    x[..., cy:cy + wy, 0:wx] = np.where(np.isnan(x[..., cy:cy + wy, 0:wx]), 1.5, x[..., cy:cy + wy, 0:wx])
    x[..., cy:cy + wy, 0] = np.nan
    if kx > 1:
        x[..., 0:wy, cx:cx + wx] = -0.0
    if ky > 1 and kx > 1:
        x[..., cy, cx] = np.inf
        x[..., cy + wy - 1, cx + wx - 1] = -np.inf
    return x


# ---- metadata and the calls that have to raise ---------------------------------------------------------------------------------
def stamps(n, minutes=5):
    t0 = datetime.datetime(2021, 6, 1, 12, 0)
    return [t0 + datetime.timedelta(minutes=minutes * i) for i in range(n)]


def geo(m, n, **more):
    meta = {"x1": 0.0, "x2": float(n), "y1": 0.0, "y2": float(m), "xpixelsize": 1.0, "ypixelsize": 1.0, "yorigin": "upper",
            "zerovalue": -15.0, "unit": "mm/h"}
    meta.update(more)
    return meta


def bad_calls():
    """(id, fn, args, kwargs): calls the reference answers with an exception."""
    x3 = np.zeros((6, 4, 5))
    t6 = {"unit": "mm/h", "timestamps": stamps(6)}
    return [
        ("agg_axis_2d", "aggregate_fields", (x3, 2), {"axis": [[0, 1]]}),
        ("agg_shapes", "aggregate_fields", (x3, (2, 2, 2)), {"axis": (0, 1)}),
        ("agg_windows_for_one_axis", "aggregate_fields", (x3, (2, 2)), {"axis": 0}),
        ("agg_method", "aggregate_fields", (x3, 2), {"method": "median"}),
        ("agg_window_zero", "aggregate_fields", (x3, 0), {}),
        ("agg_not_divisible", "aggregate_fields", (x3, 4), {}),
        ("time_2d", "aggregate_fields_time", (np.zeros((4, 5)), t6, 10), {}),
        ("time_5d", "aggregate_fields_time", (np.zeros((1, 1, 6, 4, 5)), t6, 10), {}),
        ("time_stamps", "aggregate_fields_time", (np.zeros((5, 4, 5)), t6, 10), {}),
        ("time_split", "aggregate_fields_time", (x3, t6, 20), {}),
        ("time_unit", "aggregate_fields_time", (x3, dict(t6, unit="dBZ"), 10), {}),
        ("space_1d", "aggregate_fields_space", (np.zeros(6), geo(6, 6), 2), {}),
        ("space_5d", "aggregate_fields_space", (np.zeros((1, 1, 1, 6, 6)), geo(6, 6), 2), {}),
        ("space_split", "aggregate_fields_space", (np.zeros((6, 6)), geo(6, 6), 4), {}),
        ("space_unit", "aggregate_fields_space", (np.zeros((6, 6)), geo(6, 6, unit="dBZ"), 2), {}),
        ("clip_1d", "clip_domain", (np.zeros(6), geo(6, 6), (1, 3, 1, 3)), {}),
        ("clip_5d", "clip_domain", (np.zeros((1, 1, 1, 6, 6)), geo(6, 6), (1, 3, 1, 3)), {}),
        ("square_1d", "square_domain", (np.zeros(6), geo(6, 6)), {}),
        ("square_5d", "square_domain", (np.zeros((1, 1, 1, 6, 8)), geo(6, 8)), {}),
        ("square_method", "square_domain", (np.zeros((6, 8)), geo(6, 8)), {"method": "stretch"}),
        ("square_inverse_1d", "square_domain", (np.zeros(6), geo(6, 6)), {"inverse": True}),
        ("square_inverse_5d", "square_domain", (np.zeros((1, 1, 1, 6, 8)), geo(6, 8)), {"inverse": True}),
    ]


# ---- the restatement -------------------------------------------------------------------------------------------------------
def aggregate(x, w, axis=0, method="mean", trim=False):
    """``aggregate_fields`` for one axis with the order written out: starting from +0 (NumPy's identity: a window of
    -0.0 sums to +0.0) the entries are added one by one in index order, in the array's dtype; the nan* methods add +0 for a NaN; mean / nanmean divide by the
    window size / the count of non-NaN entries in float64 and store the quotient in the array's dtype."""
    x = np.asarray(x)
    axis %= x.ndim
    n = x.shape[axis]
    if n % w and not trim:
        raise ValueError("window does not divide the axis")
    K = n // w
    v = np.moveaxis(x, axis, 0)[:K * w]
    v = v.reshape((K, w) + v.shape[1:])
    skip = method in ("nansum", "nanmean")
    acc = cnt = None
    for i in range(w):
        t = v[:, i]
        ok = ~np.isnan(t)
        if skip:
            t = np.where(ok, t, x.dtype.type(0))
        acc = (np.zeros_like(t) if i == 0 else acc) + t
        cnt = ok.astype(np.int64) if i == 0 else cnt + ok
    assert acc.dtype == x.dtype
    if method in ("mean", "nanmean"):
        with np.errstate(invalid="ignore", divide="ignore"):
            acc = (acc.astype(np.float64) / (np.float64(w) if method == "mean" else cnt)).astype(x.dtype)
    return np.ascontiguousarray(np.moveaxis(acc, 0, axis))


def upscale(x, wy, wx, ignore_nan=False):
    """``aggregate_fields_space``'s arithmetic: the (nan)mean over wy rows, rounded, then over wx of those."""
    method = "nanmean" if ignore_nan else "mean"
    return aggregate(aggregate(x, wy, x.ndim - 2, method), wx, x.ndim - 1, method)


def reordered_sums(x, w, axis):
    """nansum of every window in reversed order and as a pairwise tree (halves, recursively)."""
    x = np.asarray(x)
    K = x.shape[axis] // w
    v = np.moveaxis(x, axis, 0)[:K * w]
    v = v.reshape((K, w) + v.shape[1:])
    v = np.where(np.isnan(v), x.dtype.type(0), v)

    def tree(lo, hi):
        if hi - lo == 1:
            return v[:, lo]
        mid = (lo + hi) // 2
        return tree(lo, mid) + tree(mid, hi)

    back = v[:, w - 1].copy()
    for i in range(w - 2, -1, -1):
        back = back + v[:, i]
    return np.moveaxis(back, 0, axis), np.moveaxis(tree(0, w), 0, axis)


# ---- comparison ------------------------------------------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def mismatch(got, want):
    """None if ``got`` is ``want`` under the rule above, else a sentence."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return "shape / dtype %s %s, expected %s %s" % (got.shape, got.dtype, want.shape, want.dtype)
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    if not np.array_equal(nan_g, nan_w):
        return "%d elements are NaN on one side only, first at %s" % (
            np.count_nonzero(nan_g != nan_w), tuple(int(i) for i in np.argwhere(nan_g != nan_w)[0]))
    diff = (bits(got) != bits(want)) & ~nan_w
    if diff.any():
        at = tuple(int(i) for i in np.argwhere(diff)[0])
        return "%d elements differ in bits, first at %s: %r, expected %r" % (np.count_nonzero(diff), at, got[at], want[at])
    return None


# ---- the golden file -------------------------------------------------------------------------------------------------------
def encode_meta(meta):
    def enc(v):
        if isinstance(v, (list, tuple, np.ndarray)) and len(v) and isinstance(v[0], datetime.datetime):
            return {"__datetimes__": [t.isoformat() for t in v]}
        if isinstance(v, (list, tuple, np.ndarray)):
            return [enc(e) for e in v]
        if isinstance(v, np.generic):
            return v.item()
        return v

    return json.dumps({k: enc(v) for k, v in meta.items()}, sort_keys=True)


def decode_meta(text):
    def dec(v):
        if isinstance(v, dict) and "__datetimes__" in v:
            return [datetime.datetime.fromisoformat(t) for t in v["__datetimes__"]]
        return v

    return {k: dec(v) for k, v in json.loads(text).items()}


def same_meta(got, want):
    """Metadata as the golden file can hold it: tuples read as lists, NumPy scalars as Python numbers."""
    return json.loads(encode_meta(got)) == json.loads(encode_meta(want))


def load_golden():
    return np.load(GOLDEN, allow_pickle=False)


def golden_calls(gold, fn=None):
    """The recorded calls: dicts with ``id``, ``fn``, ``kwargs``, ``meta`` (None for aggregate_fields) and ``returns``
    ("array", "pair" or "array_alone")."""
    calls = json.loads(str(gold["calls"]))
    return [c for c in calls if fn is None or c["fn"] == fn]


def golden_meta(call):
    return None if call["meta"] is None else decode_meta(call["meta"])


def golden_kwargs(call):
    kw = dict(call["kwargs"])
    for key in ("window_size", "axis", "extent", "space_window"):
        if isinstance(kw.get(key), list):
            kw[key] = tuple(kw[key])
    return kw
