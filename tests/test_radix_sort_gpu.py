"""The shared key-only radix sort (csrc/radix_sort.h) against NumPy, through the two entry points that make it fully
observable: psh_nqt_count_le_dev (counts, the sorted table, n_valid, min, max) and psh_blend_dense_rank_dev (dense
ranks, their number).  Everything is integer work: every comparison is exact.

The cases of helpers/radix_cases.py isolate what the rain fields of the neighbouring tests leave unvisited: one running
pass, two running passes (stability across lanes, waves and tiles), wave rounds that are digit-uniform or not, tiles
and wave quarters of one key, and the tilings past the floor - grown ``per``, kMaxTiles tiles.
tests/test_radix_cases_cpu.py proves that each case reaches what its name says."""

import ctypes

import numpy as np
import pytest

from helpers import blending as hb
from helpers import radix_cases as rc

pytestmark = pytest.mark.gpu

SMALL = rc.small_cases()
SEVERAL = rc.several_tile_cases()
LARGE = rc.large_cases()
NAN_EDGES = rc.nan_edge_cases()
# run by test_large_bits_twice_then_small_cases, which also repeats it
REPEATED = "bits-max-tiles"


def _dev(a):
    from pysteps_amd.device import DeviceArray

    return DeviceArray.from_host(np.ascontiguousarray(a))


def _count_le(x, stage=None):
    """(counts, sorted values, number of values that are not NaN, min, max) from psh_nqt_count_le_dev."""
    from pysteps_amd import _lib
    from pysteps_amd.device import DeviceArray

    d_x = _dev(x)
    count = DeviceArray(x.shape, np.uint32)
    ordered = DeviceArray(x.shape, x.dtype)
    n_valid, lo, hi = ctypes.c_size_t(), ctypes.c_double(), ctypes.c_double()
    _lib.check(_lib.lib().psh_nqt_count_le_dev(d_x.ptr, int(x.dtype == np.float32), x.size, count.ptr, ordered.ptr,
                                               ctypes.byref(n_valid), ctypes.byref(lo), ctypes.byref(hi), stage),
               "psh_nqt_count_le_dev")
    return count.to_host(), ordered.to_host(), n_valid.value, lo.value, hi.value


def _dense_rank(x):
    from pysteps_amd import _lib
    from pysteps_amd.device import DeviceArray

    d_x = _dev(x)
    rank = DeviceArray(x.shape, np.uint32)
    distinct = ctypes.c_uint(0)
    _lib.check(_lib.lib().psh_blend_dense_rank_dev(d_x.ptr, int(x.dtype == np.float32), x.size, rank.ptr, ctypes.byref(distinct)),
               "psh_blend_dense_rank_dev")
    return rank.to_host(), distinct.value


def _bits(a):
    return np.ascontiguousarray(a).view(rc.key_dtype(a.dtype)) if a.dtype.kind == "f" else a


def _same(what, got, want, n, wrong=None):
    """Assert got == want element by element; the message places the first difference in the sort's tiling of n keys."""
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s, want %s %s" % (what, got.shape, got.dtype, want.shape, want.dtype)
    if wrong is None:
        wrong = _bits(got) != _bits(want)
    where = np.flatnonzero(wrong)
    if where.size:
        i = int(where[0])
        per, tiles = rc.tiling(n)
        tile, quarter, rnd = rc.place(i, n)
        pytest.fail("%s: %d of %d elements differ; the first at index %d = tile %d of %d (%d keys a tile), wave quarter %d, round %d, "
                    "lane %d: got %r, want %r" % (what, where.size, got.size, i, tile, tiles, per, quarter, rnd, i % rc.WAVE,
                                                  got[i], want[i]))


def _same_number(what, got, want):
    assert got == want or (got != got and want != want), "%s: got %r, want %r" % (what, got, want)


def _hold_count_le(tag, x, oracle, out):
    count, ordered, n_valid, lo, hi = out
    n = x.size
    assert n_valid == oracle.n_valid, "%s: n_valid %d, want %d" % (tag, n_valid, oracle.n_valid)
    head, want = ordered[:n_valid], oracle.sorted
    # the sort's own output first.  The same values, and the same bits except that a -0.0 may come back as +0.0
    _same(tag + " sorted table (output order)", head, want, n, wrong=(head != want) | ((want != 0) & (_bits(head) != _bits(want))))
    assert np.all(np.isnan(ordered[n_valid:])), "%s: %d of the %d entries behind the values are not NaN" % (
        tag, np.count_nonzero(~np.isnan(ordered[n_valid:])), n - n_valid)
    _same(tag + " counts (input order)", count, oracle.count, n)
    _same_number(tag + " min", lo, oracle.min)
    _same_number(tag + " max", hi, oracle.max)


def _hold_rank(tag, x, oracle, out):
    rank, distinct = out
    assert distinct == oracle.distinct, "%s: %d distinct values, want %d" % (tag, distinct, oracle.distinct)
    _same(tag + " dense ranks (input order)", rank, oracle.rank, x.size)


def _hold(case, x, oracle=None):
    """Both entry points on the case's values against one oracle; returns what the device gave."""
    oracle = oracle if oracle is not None else rc.Oracle(x)
    out = {"count_le": _count_le(x)}
    _hold_count_le("%s count_le" % case.id, x, oracle, out["count_le"])
    if not case.nan:
        out["rank"] = _dense_rank(x)
        _hold_rank("%s rank" % case.id, x, oracle, out["rank"])
    return out


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("family", sorted(SMALL))
def test_small_sizes(family, dtype):
    """One key, one wave round and one key more, one block round, a wave quarter of one key, three quarters, a tile, a
    tile of one key, two tiles."""
    for case in SMALL[family][dtype]:
        x, _ = case.build()
        _hold(case, x)


@pytest.mark.parametrize("case", SEVERAL, ids=lambda c: c.id)
def test_several_tiles(case):
    """35 tiles at the floor: one running pass per digit, every pair of running passes, runs of equal keys with and
    against the wave rounds, the signed mixture, NaN and infinities."""
    x, _ = case.build()
    _hold(case, x)


@pytest.mark.parametrize("case", NAN_EDGES, ids=lambda c: c.id)
def test_nan_edges(case):
    x, _ = case.build()
    out = _hold(case, x)
    if case.name == "all-nan":
        count, ordered, n_valid, lo, hi = out["count_le"]
        assert n_valid == 0 and not count.any() and np.all(np.isnan(ordered)) and lo != lo and hi != hi


@pytest.mark.parametrize("case", [c for c in LARGE if c.name != REPEATED], ids=lambda c: c.id)
def test_tiling_regimes(case):
    """All tiles full at the floor, the first grown ``per``, kMaxTiles tiles of it, the next ``per``."""
    x, _ = case.build()
    assert rc.tiling(x.size) == (case.claims["per"], case.claims["tiles"])
    _hold(case, x)


@pytest.mark.parametrize("dtype", rc.DTYPES, ids=["float32", "float64"])
def test_large_bits_twice_then_small_cases(dtype):
    """kMaxTiles tiles of random bit patterns, twice: the same bits both times.  Then, in the workspace and the
    (digit, tile) table that run left behind, a tile of one key and a several-tile case against their oracles."""
    case = rc.find(LARGE, REPEATED, dtype)
    x, _ = case.build()
    assert rc.tiling(x.size)[1] == rc.K_MAX_TILES
    oracle = rc.Oracle(x)
    first = _hold(case, x, oracle)
    again = {"count_le": _count_le(x), "rank": _dense_rank(x)}
    _same("repeat: counts", again["count_le"][0], first["count_le"][0], x.size)
    _same("repeat: sorted table", again["count_le"][1], first["count_le"][1], x.size)
    assert again["count_le"][2:] == first["count_le"][2:]
    _same("repeat: ranks", again["rank"][0], first["rank"][0], x.size)
    assert again["rank"][1] == first["rank"][1]
    del x, oracle, first, again
    D = rc.digits_of(dtype)
    small = [c for c in SMALL["bits"][np.dtype(dtype).name] if c.claims["n"] == rc.N_ONE_KEY_TILE]
    assert len(small) == 1
    for follow in (small[0], rc.find(SEVERAL, "digits-0-%d" % (D - 1), dtype), rc.find(SEVERAL, "runs64-shift32", dtype)):
        y, _ = follow.build()
        _hold(follow, y)


def test_stage_times_do_not_change_the_outputs():
    case = rc.find(SEVERAL, "digits-0-3", np.float32)
    x, _ = case.build()
    oracle = rc.Oracle(x)
    stage = (ctypes.c_float * 3)(-1.0, -1.0, -1.0)
    _hold_count_le("%s count_le with stage_ms" % case.id, x, oracle, _count_le(x, stage))
    times = list(stage)
    print("stage_ms: keys and histograms %.4f, sort passes %.4f, counts and table %.4f" % tuple(times))
    assert all(np.isfinite(t) and t >= 0.0 for t in times), times


def _salient_inputs():
    m, n = 1449, 1448
    assert rc.tiling(2 * m * n)[0] > rc.K_MIN_TILE
    rng = np.random.default_rng(91)
    return hb.rain(rng, (2, 1, m, n)).astype(np.float32), hb.rain(rng, (2, 1, m, n)).astype(np.float32)


def test_salient_blend_in_the_grown_tiling():
    """Two member pairs of 1449 x 1448: the ranks of 4 196 304 keys in one sort with grown tiles feed the salient blend.
    One wrong rank is one wrong pixel."""
    from pysteps_amd.blending import linear_blending
    from pysteps_amd.device import DeviceArray

    nowcast, nwp = _salient_inputs()
    schedule = dict(timesteps=1, timestep=5, start_blending=0, end_blending=10)  # one lead time, NWP weight 1 / 2
    assert hb.weights(**schedule) == [0.5]
    got = linear_blending.blend(_dev(nowcast), _dev(nwp), saliency=True, **schedule)
    assert isinstance(got, DeviceArray)
    got = got.to_host()
    want = hb.blend(nowcast, nwp, saliency=True, **schedule)
    assert not np.isnan(want).any() and np.count_nonzero(want) > want.size // 20
    _same("salient blend (pixel order of the two planes)", got.ravel(), want.ravel(), want.size)
