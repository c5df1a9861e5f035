"""Cases and the oracle for the key-only LSD radix sort of pysteps_amd/csrc/radix_sort.h, which nqt.hip
(psh_nqt_count_le_dev) and blending.hip (psh_blend_dense_rank_dev) share.

The sort's constants are read from the header, ``tiling`` is restated from them and every size below is derived from the
parsed values, so the cases follow a change of the constants; tests/test_radix_cases_cpu.py proves on the CPU that each
case reaches the regime, the digit set and the round pattern its name claims.

Rounds.  Every kernel of a pass reads a tile in rounds of 64 keys per wave.  ``per`` is a multiple of kThreads and the wave
quarter ``per / kWaves`` a multiple of 64, so a round always starts at a multiple of 64 of the whole array, in
hist_all / pass_count (256 keys a block round) and in pass_scatter (64 keys a wave round) alike.  The full rounds of an
array of n keys are therefore its first n // 64 chunks of 64 keys, whatever the tiling; the last n % 64 keys are the one
partial round.  A full round whose keys share the pass's digit takes hist_add's ``+64`` path.

Digit-prescribed cases are built as integer keys around the key of 1.5 and turned into values with ``key_value``.  Keys
that come out NaN or -0.0 (whose key is that of 0.0, another digit pattern) are dropped, and so are the few that come out
infinite, because the rank entry point takes finite values only.  DROP_CAP bounds the dropped share of a case.

One oracle per case serves both entry points: ``np.unique`` with inverse and counts."""

import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HEADER = os.path.join(ROOT, "pysteps_amd", "csrc", "radix_sort.h")
F32, F64 = np.float32, np.float64
DTYPES = (F32, F64)
WAVE = 64
DROP_CAP = 0.01


def _constant(text, name):
    found = re.findall(r"constexpr\s+(?:int|size_t|unsigned)\s+%s\s*=\s*(\d+)\s*;" % name, text)
    assert len(found) == 1, "%s: %d definitions of %s" % (HEADER, len(found), name)
    return int(found[0])


def constants():
    """(kThreads, kMaxTiles, kMinTile) as radix_sort.h defines them."""
    with open(HEADER) as fh:
        text = fh.read()
    assert re.search(r"constexpr\s+int\s+kWaves\s*=\s*kThreads\s*/\s*64\s*;", text), "kWaves is no longer kThreads / 64"
    return tuple(_constant(text, name) for name in ("kThreads", "kMaxTiles", "kMinTile"))


K_THREADS, K_MAX_TILES, K_MIN_TILE = constants()
K_WAVES = K_THREADS // WAVE
assert K_THREADS % WAVE == 0 and K_MIN_TILE % K_THREADS == 0 and K_MAX_TILES % K_THREADS == 0


def tiling(n):
    """``(per, tiles)`` of radix_sort.h: per = max(kMinTile, align_up(ceil(n / kMaxTiles), kThreads))."""
    share = (n + K_MAX_TILES - 1) // K_MAX_TILES
    per = max(K_MIN_TILE, (share + K_THREADS - 1) // K_THREADS * K_THREADS)
    return per, (n + per - 1) // per


def last_tile(n):
    per, tiles = tiling(n)
    return n - (tiles - 1) * per


def place(i, n):
    """Where element i of n keys is read by a pass: (tile, wave quarter, round of that wave)."""
    per, _ = tiling(n)
    in_tile = i % per
    wlen = per // K_WAVES
    return i // per, in_tile // wlen, (in_tile % wlen) // WAVE


# ---- sizes, from the constants ------------------------------------------------------------------------------------------
QUARTER = K_MIN_TILE // K_WAVES
SMALL_SIZES = (1, 2, WAVE - 1, WAVE, WAVE + 1, K_THREADS - 1, K_THREADS, K_THREADS + 1, QUARTER - 1, QUARTER, QUARTER + 1,
               3 * QUARTER - 1, 3 * QUARTER, 3 * QUARTER + 1, K_MIN_TILE - 1, K_MIN_TILE, K_MIN_TILE + 1, 2 * K_MIN_TILE - 1,
               2 * K_MIN_TILE + 1)
N_ONE_KEY_TILE = K_MIN_TILE + 1  # the second tile holds one key: waves 1..3 of it are empty
N_SEVERAL = 34 * K_MIN_TILE + 5 * WAVE + 49  # 35 tiles at the floor, a partial last tile and a partial last wave round
N_FLOOR_FULL = K_MIN_TILE * K_MAX_TILES  # the last n at the floor: kMaxTiles tiles, all full
N_FIRST_GROWN = N_FLOOR_FULL + 1  # the first n with per > kMinTile
PER_GROWN = K_MIN_TILE + K_THREADS
N_MAX_TILES = PER_GROWN * K_MAX_TILES - 1  # kMaxTiles tiles of the grown per, the last one a key short
N_NEXT_PER = PER_GROWN * K_MAX_TILES + 1  # the first n of the next per
# name -> (n, per, tiles, keys of the last tile), the table of the regimes as the constants give it
REGIMES = {
    "floor-full": (N_FLOOR_FULL, K_MIN_TILE, K_MAX_TILES, K_MIN_TILE),
    "first-grown": (N_FIRST_GROWN, PER_GROWN, (N_FIRST_GROWN + PER_GROWN - 1) // PER_GROWN,
                    N_FIRST_GROWN - (N_FIRST_GROWN - 1) // PER_GROWN * PER_GROWN),
    "max-tiles": (N_MAX_TILES, PER_GROWN, K_MAX_TILES, PER_GROWN - 1),
    "next-per": (N_NEXT_PER, PER_GROWN + K_THREADS, (N_NEXT_PER + PER_GROWN + K_THREADS - 1) // (PER_GROWN + K_THREADS),
                 N_NEXT_PER - (N_NEXT_PER - 1) // (PER_GROWN + K_THREADS) * (PER_GROWN + K_THREADS)),
}


# ---- keys and back ------------------------------------------------------------------------------------------------------
def key_dtype(dtype):
    return np.uint32 if np.dtype(dtype) == F32 else np.uint64


def digits_of(dtype):
    return np.dtype(dtype).itemsize


def okey(x):
    """The order-preserving integer image of radix_sort.h; -0.0 and 0.0 share one key."""
    x = np.ascontiguousarray(x)
    kt = key_dtype(x.dtype)
    bits = 8 * x.dtype.itemsize
    b = np.where(x == 0, x.dtype.type(0.0), x).view(kt)
    top = kt(1 << (bits - 1))
    return np.where(b & top != 0, ~b, b | top)


def key_value(k, dtype):
    """The value whose key is k (the inverse of ``okey`` away from -0.0)."""
    kt = key_dtype(dtype)
    k = np.ascontiguousarray(k, dtype=kt)
    top = kt(1 << (8 * k.dtype.itemsize - 1))
    return np.where(k & top != 0, k & ~top, ~k).view(dtype)


def digit(keys, d):
    return ((keys >> keys.dtype.type(8 * d)) & keys.dtype.type(255)).astype(np.uint8)


def varying_digits(keys):
    return {d for d in range(keys.dtype.itemsize) if np.any(digit(keys, d) != digit(keys[:1], d))}


def round_uniformity(keys, d):
    """For every full round (see the module's docstring): do its 64 keys share digit d?"""
    full = len(keys) // WAVE
    rounds = digit(keys[:full * WAVE], d).reshape(full, WAVE)
    return np.all(rounds == rounds[:, :1], axis=1)


def with_digits(base_key, columns, dtype):
    """Keys equal to base_key but for the bytes given: ``columns`` maps a digit to an array of its values."""
    kt = key_dtype(dtype)
    n = len(next(iter(columns.values())))
    keys = np.full(n, base_key, dtype=kt)
    for d, col in columns.items():
        keys &= ~kt(255 << (8 * d))
        keys |= col.astype(kt) << kt(8 * d)
    return keys


def usable(values):
    """The elements a digit-prescribed case keeps: not NaN, not -0.0, not infinite."""
    return np.isfinite(values) & ~((values == 0) & np.signbit(values))


# ---- the oracle ---------------------------------------------------------------------------------------------------------
class Oracle:
    """What both entry points must give for x (NaN allowed): by ``np.unique`` on the values that are not NaN."""

    def __init__(self, x):
        flat = np.ascontiguousarray(x).ravel()
        ok = ~np.isnan(flat)
        valid = flat[ok]
        values, inverse, counts = np.unique(valid, return_inverse=True, return_counts=True)
        inverse = inverse.reshape(-1)
        self.n_valid = int(valid.size)
        self.distinct = int(values.size)
        self.has_nan = self.n_valid != flat.size
        self.rank = (inverse + 1).astype(np.uint32)  # of the valid values; the rank route takes no NaN
        self.count = np.zeros(flat.size, np.uint32)
        self.count[ok] = np.cumsum(counts)[inverse]
        self.sorted = np.sort(valid)
        self.min = float(self.sorted[0]) if self.n_valid else float("nan")
        self.max = float(self.sorted[-1]) if self.n_valid else float("nan")


# ---- families -----------------------------------------------------------------------------------------------------------
def _bit_patterns(rng, n, dtype):
    kt = key_dtype(dtype)
    return rng.integers(0, np.iinfo(kt).max, n, dtype=kt, endpoint=True).view(dtype)


def bits(n, dtype, seed):
    """Uniformly random bit patterns: both signs, the whole exponent range, denormals, +-0.0.  A NaN or infinite pattern
    loses its exponent bits and becomes a denormal."""
    rng = np.random.default_rng(seed)
    x = _bit_patterns(rng, n, dtype)
    kt = key_dtype(dtype)
    mantissa_bits = np.finfo(dtype).nmant
    sign_and_mantissa = kt((1 << (8 * x.dtype.itemsize - 1)) | ((1 << mantissa_bits) - 1))
    raw = x.view(kt)
    return np.where(np.isfinite(x), raw, raw & sign_and_mantissa).view(dtype)


def bits_nan(n, dtype, seed):
    """``bits`` for the count route: 1 % NaN (at least one from two keys on, never all), +-inf planted."""
    rng = np.random.default_rng(seed + 7)
    x = bits(n, dtype, seed).copy()
    if n >= 4:
        x[rng.integers(0, n, 2 + n // 1000)] = np.inf
        x[rng.integers(0, n, 2 + n // 1000)] = -np.inf
    x[rng.random(n) < 0.01] = np.nan
    if n >= 2:
        where = int(rng.integers(0, n))
        x[where] = np.nan
        if np.all(np.isnan(x)):
            x[(where + 1) % n] = dtype(1.5)
    return x


def dry(n, dtype, seed):
    """93 % one value, the rest a gamma law quantised to 1 / 8, interleaved at random."""
    rng = np.random.default_rng(seed)
    return np.where(rng.random(n) < 0.93, 0.0, np.round(rng.gamma(0.6, 4.0, n) * 8.0) / 8.0).astype(dtype)


def equal_but_last(n, dtype):
    """Every key 2.5 but the last, -3.0, whose key differs from that of 2.5 in every digit."""
    x = np.full(n, 2.5, dtype)
    x[-1] = -3.0
    return x


def signed(n, dtype, seed, inf=False):
    """Both signs, -0.0 with 0.0, neighbours in the last bit, +-max and tiny; +-inf on request (count route only)."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * 1e3).astype(dtype)
    x[::7] = -0.0
    x[1::7] = 0.0
    x[2::7] = np.nextafter(dtype(1.0), dtype(2.0))
    x[3::7] = 1.0
    x[4::97] = np.finfo(dtype).max
    x[5::97] = -np.finfo(dtype).max
    x[6::97] = np.finfo(dtype).tiny
    if inf:
        x[11::193] = np.inf
        x[12::193] = -np.inf
    return x


def base_key(dtype):
    return int(okey(np.array([1.5], dtype))[0])


def digit_case(varying, n, dtype, seed, exact=False):
    """Keys around that of 1.5 whose bytes ``varying`` are uniformly random and whose other bytes are constant.
    Returns ``(values, dropped share)``.  ``n`` counts the keys before dropping; with ``exact`` it is the number of
    values after dropping (more keys are drawn, the first n usable ones are kept)."""
    rng = np.random.default_rng(seed)
    drawn = n + n // 50 if exact else n
    keys = with_digits(base_key(dtype), {d: rng.integers(0, 256, drawn, dtype=np.uint16) for d in varying}, dtype)
    values = key_value(keys, dtype)
    keep = usable(values)
    share = 1.0 - np.count_nonzero(keep) / drawn
    values = values[keep]
    if exact:
        assert values.size >= n, "digit_case: %d usable keys of %d drawn, %d wanted" % (values.size, drawn, n)
        values = values[:n]
    return np.ascontiguousarray(values), share


def run_values(count, dtype, seed):
    """``count`` distinct values in random order.  Bytes 0, 1 and 2 of their keys vary, so three passes run, and no two
    consecutive values share any of the three: a round that holds two runs is uniform in no running pass."""
    rng = np.random.default_rng(seed)
    varying = (0, 1, 2)
    seen, rows = set(), []
    previous = (-1, -1, -1)
    while len(rows) < count:
        row = tuple(int(v) for v in rng.integers(0, 256, len(varying)))
        if row in seen or any(a == b for a, b in zip(row, previous)):
            continue
        seen.add(row)
        rows.append(row)
        previous = row
    columns = np.array(rows, dtype=np.uint16)
    keys = with_digits(base_key(dtype), {d: columns[:, j] for j, d in enumerate(varying)}, dtype)
    values = key_value(keys, dtype)
    assert np.all(usable(values)) and np.unique(values).size == count
    return values


def runs(n, dtype, seed, length, shift=0):
    """Consecutive runs of ``length`` equal values, distinct between runs; ``shift`` keys of one more value in front."""
    count = (n + length - 1) // length + 1
    values = run_values(count, dtype, seed)
    x = np.concatenate([np.full(shift, values[0], dtype), np.repeat(values[1:], length)])[:n]
    assert x.size == n
    return np.ascontiguousarray(x)


class Case:
    """A named input.  ``build()`` returns the values; ``nan``: count route only; ``claims``: what the CPU test proves."""

    def __init__(self, name, dtype, build, nan=False, **claims):
        self.name, self.dtype, self._build, self.nan, self.claims = name, np.dtype(dtype).type, build, nan, claims
        self.id = "%s-%s" % (name, np.dtype(dtype).name)

    def build(self):
        """(values, dropped share)."""
        out = self._build()
        x, share = out if isinstance(out, tuple) else (out, 0.0)
        assert x.dtype == self.dtype and x.ndim == 1
        return x, share

    def __repr__(self):
        return self.id


def _pairs(D):
    return [(lo, hi) for lo in range(D) for hi in range(lo + 1, D)]


def small_cases():
    """family -> dtype name -> the cases at every size of SMALL_SIZES."""
    out = {}
    for dtype in DTYPES:
        for family in ("bits", "dry", "equal-but-last", "bits-nan"):
            cases = []
            for n in SMALL_SIZES:
                if family == "bits":
                    c = Case("bits-n%d" % n, dtype, lambda n=n, dtype=dtype: bits(n, dtype, 100 + n), n=n)
                elif family == "dry":
                    c = Case("dry-n%d" % n, dtype, lambda n=n, dtype=dtype: dry(n, dtype, 200 + n), n=n)
                elif family == "equal-but-last":
                    c = Case("equal-but-last-n%d" % n, dtype, lambda n=n, dtype=dtype: equal_but_last(n, dtype), n=n,
                             partial_mixed_end=n % WAVE >= 2)
                else:
                    c = Case("bits-nan-n%d" % n, dtype, lambda n=n, dtype=dtype: bits_nan(n, dtype, 300 + n), nan=True, n=n)
                cases.append(c)
            out.setdefault(family, {})[np.dtype(dtype).name] = cases
    return out


def several_tile_cases():
    """The cases of N_SEVERAL keys: one digit, two digits, runs, the signed mixture, NaN."""
    out = []
    n = N_SEVERAL
    for dtype in DTYPES:
        D = digits_of(dtype)
        for d in range(D):
            out.append(Case("digit-%d" % d, dtype, lambda d=d, dtype=dtype: digit_case((d,), n, dtype, 400 + d), drawn=n,
                            digits={d}))
        for lo, hi in _pairs(D):
            out.append(Case("digits-%d-%d" % (lo, hi), dtype,
                            lambda lo=lo, hi=hi, dtype=dtype: digit_case((lo, hi), n, dtype, 500 + 8 * lo + hi), drawn=n,
                            digits={lo, hi}))
        out.append(Case("runs64-aligned", dtype, lambda dtype=dtype: runs(n, dtype, 600, 64), n=n, rounds="uniform"))
        out.append(Case("runs64-shift32", dtype, lambda dtype=dtype: runs(n, dtype, 601, 64, shift=32), n=n, rounds="mixed"))
        out.append(Case("runs100", dtype, lambda dtype=dtype: runs(n, dtype, 602, 100), n=n, rounds="both"))
        out.append(Case("signed", dtype, lambda dtype=dtype: signed(n, dtype, 700), n=n))
        out.append(Case("signed-inf", dtype, lambda dtype=dtype: signed(n, dtype, 701, inf=True), nan=True, n=n))
        out.append(Case("bits-nan", dtype, lambda dtype=dtype: bits_nan(n, dtype, 702), nan=True, n=n))
    return out


def large_cases():
    """``bits`` and ``dry`` in each regime of REGIMES, two digits across the first grown tiling, NaN there as well."""
    out = []
    for dtype in DTYPES:
        D = digits_of(dtype)
        for regime, (n, per, tiles, last) in REGIMES.items():
            claims = dict(n=n, per=per, tiles=tiles, last_tile=last)
            out.append(Case("bits-%s" % regime, dtype, lambda n=n, dtype=dtype: bits(n, dtype, 800), **claims))
            out.append(Case("dry-%s" % regime, dtype, lambda n=n, dtype=dtype: dry(n, dtype, 801), rounds="both", **claims))
        n, per, tiles, last = REGIMES["first-grown"]
        claims = dict(n=n, per=per, tiles=tiles, last_tile=last)
        out.append(Case("digits-0-%d-first-grown" % (D - 1), dtype,
                        lambda n=n, dtype=dtype, D=D: digit_case((0, D - 1), n, dtype, 802, exact=True), digits={0, D - 1},
                        **claims))
        out.append(Case("bits-nan-first-grown", dtype, lambda n=n, dtype=dtype: bits_nan(n, dtype, 803), nan=True, **claims))
    return out


def nan_edge_cases():
    """All NaN but one at the size whose second tile holds one key; all NaN."""
    out = []
    for dtype in DTYPES:
        def but_one(dtype=dtype):
            x = np.full(N_ONE_KEY_TILE, np.nan, dtype)
            x[N_ONE_KEY_TILE // 3] = -2.25
            return x

        out.append(Case("all-nan-but-one", dtype, but_one, nan=True, n=N_ONE_KEY_TILE))
        out.append(Case("all-nan", dtype, lambda dtype=dtype: np.full(300, np.nan, dtype), nan=True, n=300))
    return out


def find(cases, name, dtype):
    hits = [c for c in cases if c.name == name and c.dtype == np.dtype(dtype).type]
    assert len(hits) == 1, (name, dtype, hits)
    return hits[0]
