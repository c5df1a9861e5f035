"""The cases of helpers/radix_cases.py reach what their names claim (no GPU): the tiling regime, the set of digits that
vary - the passes that run -, the pattern of digit-uniform wave rounds, the cap on dropped keys, and an oracle that
agrees with ``np.searchsorted``.  The sizes are derived from the constants of radix_sort.h; if kMinTile or kMaxTiles
change and a case no longer reaches its regime, this file fails."""

import numpy as np
import pytest

from helpers import radix_cases as rc

SMALL = rc.small_cases()
SEVERAL = rc.several_tile_cases()
LARGE = rc.large_cases()
NAN_EDGES = rc.nan_edge_cases()
SMALL_FLAT = [c for by_dtype in SMALL.values() for cases in by_dtype.values() for c in cases]


def _check_rounds(case, keys):
    want = case.claims.get("rounds")
    if want is None:
        return
    running = rc.varying_digits(keys)
    assert running, case
    for d in running:
        uniform = rc.round_uniformity(keys, d)
        assert uniform.size > 100
        if want == "uniform":
            assert uniform.all(), (case, d)
        elif want == "mixed":
            assert not uniform.any(), (case, d, int(np.count_nonzero(uniform)))
        else:
            assert uniform.any() and not uniform.all(), (case, d)


def _check_claims(case, x, share):
    claims = case.claims
    assert share <= rc.DROP_CAP, "%s: %.2f %% of the keys dropped" % (case, 100 * share)
    if "n" in claims:
        assert x.size == claims["n"] and (share == 0.0 or "digits" in claims)
    if "drawn" in claims:
        assert x.size == claims["drawn"] - round(share * claims["drawn"])
    if "per" in claims:
        assert rc.tiling(x.size) == (claims["per"], claims["tiles"]) and rc.last_tile(x.size) == claims["last_tile"]
    keys = rc.okey(x[~np.isnan(x)])
    if "digits" in claims:
        assert rc.varying_digits(keys) == claims["digits"], case
        assert np.all(rc.usable(x))
        for d in claims["digits"]:  # both bytes over (nearly) all of their values: 255 where the top byte loses its NaN
            assert np.unique(rc.digit(keys, d)).size >= 255
    if not case.nan:
        assert np.all(np.isfinite(x)), case  # the rank route takes finite values only
    _check_rounds(case, keys)


def _check_oracle(x):
    oracle = rc.Oracle(x)
    ok = ~np.isnan(x)
    want = np.zeros(x.size, np.uint32)
    want[ok] = np.searchsorted(np.sort(x[ok]), x[ok], side="right")
    assert np.array_equal(oracle.count, want)
    assert oracle.n_valid == np.count_nonzero(ok)
    if oracle.n_valid:
        values, inverse = np.unique(x[ok], return_inverse=True)
        assert np.array_equal(oracle.rank, np.searchsorted(values, x[ok], side="left") + 1) and oracle.distinct == values.size
        assert oracle.min == x[ok].min() and oracle.max == x[ok].max()
    else:
        assert np.isnan(oracle.min) and np.isnan(oracle.max) and oracle.distinct == 0 and not oracle.count.any()


def test_constants_and_tiling_follow_the_header():
    assert rc.K_WAVES == 4 and rc.K_MAX_TILES // rc.K_THREADS >= 1
    for n in (1, rc.K_MIN_TILE, rc.K_MIN_TILE + 1, rc.N_FLOOR_FULL, rc.N_FIRST_GROWN, rc.N_MAX_TILES, rc.N_NEXT_PER, 4096 * 4096):
        per, tiles = rc.tiling(n)
        assert per % rc.K_THREADS == 0 and (per // rc.K_WAVES) % rc.WAVE == 0 and per >= rc.K_MIN_TILE
        assert 1 <= tiles <= rc.K_MAX_TILES and (tiles - 1) * per < n <= tiles * per
    if (rc.K_THREADS, rc.K_MAX_TILES, rc.K_MIN_TILE) == (256, 2048, 2048):  # the figures the cases were first written for
        assert rc.SMALL_SIZES == (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1535, 1536, 1537, 2047, 2048, 2049, 4095, 4097)
        assert rc.N_SEVERAL == 70001
        assert rc.REGIMES == {"floor-full": (4194304, 2048, 2048, 2048), "first-grown": (4194305, 2304, 1821, 1025),
                              "max-tiles": (4718591, 2304, 2048, 2303), "next-per": (4718593, 2560, 1844, 513)}
        assert rc.tiling(4096 * 4096) == (8192, 2048) and rc.tiling(2 * 1449 * 1448) == (2304, 1822)


def test_regimes_are_the_first_and_last_sizes_of_their_tiling():
    n, per, tiles, last = rc.REGIMES["floor-full"]
    assert rc.tiling(n) == (rc.K_MIN_TILE, rc.K_MAX_TILES) and last == per  # all tiles full, the last size at the floor
    n, per, tiles, last = rc.REGIMES["first-grown"]
    assert rc.tiling(n - 1)[0] == rc.K_MIN_TILE < rc.tiling(n)[0] == per and (per // rc.K_WAVES) > rc.QUARTER
    assert tiles < rc.K_MAX_TILES and 0 < last < per and last % rc.WAVE != 0
    n, per, tiles, last = rc.REGIMES["max-tiles"]
    assert rc.tiling(n) == (per, rc.K_MAX_TILES) and per > rc.K_MIN_TILE and last == per - 1
    n, per, tiles, last = rc.REGIMES["next-per"]
    assert rc.tiling(n - 2)[0] == rc.REGIMES["max-tiles"][1] < rc.tiling(n)[0] == per
    # the small sizes: one key in a tile, one key in a wave quarter, a several-tile size with a partial last round
    assert rc.tiling(rc.N_ONE_KEY_TILE) == (rc.K_MIN_TILE, 2) and rc.last_tile(rc.N_ONE_KEY_TILE) == 1
    assert rc.N_ONE_KEY_TILE in rc.SMALL_SIZES and rc.QUARTER + 1 in rc.SMALL_SIZES
    per, tiles = rc.tiling(rc.N_SEVERAL)
    assert per == rc.K_MIN_TILE and tiles == 35 and 0 < rc.last_tile(rc.N_SEVERAL) < rc.QUARTER and rc.N_SEVERAL % rc.WAVE != 0
    assert rc.place(rc.N_SEVERAL - 1, rc.N_SEVERAL) == (34, 0, 5) and rc.place(rc.K_MIN_TILE + rc.QUARTER, rc.N_SEVERAL) == (1, 1, 0)


@pytest.mark.parametrize("dtype", rc.DTYPES, ids=["f32", "f64"])
def test_keys_preserve_the_order_and_come_back(dtype):
    x = np.concatenate([rc.bits(20000, dtype, 1), rc.signed(5000, dtype, 2, inf=True)])
    keys = rc.okey(x)
    order = np.argsort(x, kind="stable")
    assert np.all(keys[order][1:] >= keys[order][:-1])
    assert np.array_equal(keys[order][1:] == keys[order][:-1], x[order][1:] == x[order][:-1])
    back = rc.key_value(keys, dtype)
    assert np.array_equal(back, x) and np.array_equal(np.signbit(back)[x != 0], np.signbit(x)[x != 0])
    assert not np.signbit(back[x == 0]).any()  # -0.0 folded onto 0.0
    nan_key = np.array([~np.uint64(0)]).astype(rc.key_dtype(dtype))  # the key nqt.hip gives a NaN
    assert np.isnan(rc.key_value(nan_key, dtype)[0]) and np.all(keys < nan_key[0])
    assert rc.key_value(np.array([rc.base_key(dtype)]), dtype)[0] == 1.5


@pytest.mark.parametrize("case", SMALL_FLAT + SEVERAL + NAN_EDGES, ids=lambda c: c.id)
def test_small_and_several_tile_cases(case):
    x, share = case.build()
    again, _ = case.build()
    assert np.array_equal(x.view(rc.key_dtype(case.dtype)), again.view(rc.key_dtype(case.dtype)))  # rebuilt from its recipe
    _check_claims(case, x, share)
    _check_oracle(x)
    if case.name.startswith("equal-but-last"):
        keys = rc.okey(x)
        assert x.size == 1 or rc.varying_digits(keys) == set(range(rc.digits_of(case.dtype)))  # every pass runs
        tail = x.size % rc.WAVE
        assert case.claims["partial_mixed_end"] == (tail >= 2)
        if tail >= 2:  # full rounds all uniform, the last round partial and mixed
            assert all(rc.round_uniformity(keys, d).all() for d in range(keys.dtype.itemsize))
            assert keys[-1] != keys[-2] == keys[-tail]
    if case.name == "runs64-aligned":  # the last round: fewer than 64 keys that share every digit - hist_add's per-lane path
        tail = x.size % rc.WAVE
        assert tail >= 2 and np.all(x[-tail:] == x[-1]) and x[-tail - 1] != x[-1]
    if case.nan and case.name.startswith(("bits-nan", "signed-inf")):
        assert x.size < 4 or np.isinf(x).any()
        if case.name.startswith("bits-nan"):
            assert x.size < 2 or (np.isnan(x).any() and not np.isnan(x).all())


def test_equal_but_last_ends_in_a_partial_round_at_most_sizes():
    """A size that is a multiple of 64 has no partial round, and one key past a multiple leaves the odd key alone in it:
    14 of the 19 sizes end in a partial round, in 7 of them it is mixed."""
    cases = SMALL["equal-but-last"]["float32"]
    assert sum(c.claims["n"] % rc.WAVE != 0 for c in cases) >= 14 and sum(c.claims["partial_mixed_end"] for c in cases) >= 7


@pytest.mark.parametrize("case", LARGE, ids=lambda c: c.id)
def test_large_cases(case):
    x, share = case.build()
    _check_claims(case, x, share)
    if case.nan:
        nans = np.count_nonzero(np.isnan(x))
        assert 0.008 * x.size < nans < 0.012 * x.size and np.isinf(x).any()


def test_the_case_lists_are_complete():
    for dtype in rc.DTYPES:
        D = rc.digits_of(dtype)
        names = [c.name for c in SEVERAL if c.dtype == dtype]
        assert len(names) == len(set(names))
        assert sum(n.startswith("digit-") for n in names) == D and sum(n.startswith("digits-") for n in names) == D * (D - 1) // 2
        assert {"runs64-aligned", "runs64-shift32", "runs100", "signed", "signed-inf", "bits-nan"} <= set(names)
        large = [c.name for c in LARGE if c.dtype == dtype]
        assert {"%s-%s" % (f, r) for f in ("bits", "dry") for r in rc.REGIMES} <= set(large)
        assert "digits-0-%d-first-grown" % (D - 1) in large and "bits-nan-first-grown" in large
        for family in ("bits", "dry", "equal-but-last", "bits-nan"):
            assert [c.claims["n"] for c in SMALL[family][np.dtype(dtype).name]] == list(rc.SMALL_SIZES)
